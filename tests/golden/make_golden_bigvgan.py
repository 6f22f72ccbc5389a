#!/usr/bin/env python3
"""Generate tests/golden/g23_bigvgan.npz by running the REAL reference generator, ``nvidia_bigvgan/bigvgan.py`` (BigVGAN, AMPBlock1,
AMPBlock2), on the CPU.

Run where the reference tree is available (default /root/reference, or the first argument):

    python tests/golden/make_golden_bigvgan.py

How the reference is loaded: as tests/golden/make_golden_anti_alias.py loads its modules - ``nvidia_bigvgan``, ``.alias_free_activation``
and ``.alias_free_activation.torch`` are registered as EMPTY stand-in packages (under the name ``ref_bigvgan``) whose ``__path__`` points
at the real directories - plus a stand-in for ``ref_bigvgan.utils`` made here: the real one imports matplotlib and, through
``meldataset``, librosa, and the generator uses two helpers of it: ``init_weights`` (nothing here: every weight is overwritten) and
``get_padding`` (the "same" padding ``(k - 1) d / 2``).  ``bigvgan.py``, ``activations.py``, ``env.py`` and the resampling modules are the
reference's files.  The output is data only.

Parameters (the reference's ``init_weights`` std of 0.01 would make every output vanish): weights ``randn / sqrt(fan_in)`` (fan_in of a
transposed convolution: ``C_in k``), ``alpha`` / ``beta`` ``0.3 randn``, biases ``0.1 randn``, each seeded by its state-dict key and
shape and cut to 8 significant bits (bfloat16 values): equal layers of different cases are stored once, and the file compresses.  They
are written into the model after ``remove_weight_norm()`` - except in case ``k1``, where ``weight_v`` is set, ``weight_g = |v| (0.8 ..
1.2)``, and the state dict BEFORE ``remove_weight_norm()`` is stored next to the one after it.  Inputs: ``X_SCALE randn``.

All parameters lie in ONE float32 vector ``pool``.  Per case ``<c>``: ``cases[<c>]`` (json): ``h``, the shapes, ``sd`` (state-dict key
after ``remove_weight_norm()`` -> ``[offset into pool, shape]``), for ``k1`` also ``sd_wn``; ``<c>_x`` float32; the reference in
float64 (module ``.double()``): ``<c>_y``, ``<c>_pre`` (after conv_pre),
``<c>_up<i>`` (after stage i's up-sampler), ``<c>_mean<i>`` (after stage i's mean over the blocks); ``<c>_dev32_<q>`` for each of them:
``max|q32 - q64| / max|q64|`` of the reference's own float32 run.

    amp1     rates (4,2) / kernels (8,4), AMPBlock1, snakebeta log-scale, tanh + bias      [2,8,9]
    amp2     AMPBlock2, snake linear, no tanh, no final bias                                [1,8,5]
    r8       rates (8,2) / kernels (16,4), initial channels 48                              [1,8,7]
    odd      rates (3,2) / kernels (7,4)                                                    [1,8,6]
    one      amp1's configuration                                                           [1,8,1]   (every halo longer than the signal)
    k1       a single block kernel (3,): the mean is over one block                         [1,8,4]
    pad_odd  rate 2 / kernel 5 (k - u odd: the output is one sample longer)                 [1,8,5]
(unless noted: num_mels 8, initial channels 32, block kernels (3, 7, 11), dilations (1, 3, 5))

Condition (asserted; move the seed if it fails): every ``dev32_*`` below 2e-6.
"""
import importlib
import json
import sys
import types
import zlib
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
DEV32_MAX = 2e-6
SEED = 2300
X_SCALE = 0.25

BASE = dict(num_mels=8, upsample_initial_channel=32, upsample_rates=[4, 2], upsample_kernel_sizes=[8, 4], resblock='1',
            resblock_kernel_sizes=[3, 7, 11], resblock_dilation_sizes=[[1, 3, 5], [1, 3, 5], [1, 3, 5]], activation='snakebeta',
            snake_logscale=True, use_tanh_at_final=True, use_bias_at_final=True, sampling_rate=24000)
CASES = [
    ('amp1', {}, (2, 8, 9)),
    ('amp2', dict(resblock='2', activation='snake', snake_logscale=False, use_tanh_at_final=False, use_bias_at_final=False), (1, 8, 5)),
    ('r8', dict(upsample_rates=[8, 2], upsample_kernel_sizes=[16, 4], upsample_initial_channel=48), (1, 8, 7)),
    ('odd', dict(upsample_rates=[3, 2], upsample_kernel_sizes=[7, 4]), (1, 8, 6)),
    ('one', {}, (1, 8, 1)),
    ('k1', dict(resblock_kernel_sizes=[3], resblock_dilation_sizes=[[1, 3, 5]]), (1, 8, 4)),
    ('pad_odd', dict(upsample_rates=[2], upsample_kernel_sizes=[5]), (1, 8, 5)),
]


def load_reference(root):
    import torch
    base = Path(root) / 'padertorch' / 'contrib' / 'mk' / 'synthesis' / 'vocoder' / 'nvidia_bigvgan'
    for name, path in [('ref_bigvgan', base), ('ref_bigvgan.alias_free_activation', base / 'alias_free_activation'),
                       ('ref_bigvgan.alias_free_activation.torch', base / 'alias_free_activation' / 'torch')]:
        pkg = types.ModuleType(name)
        pkg.__path__ = [str(path)]
        sys.modules[name] = pkg
    utils = types.ModuleType('ref_bigvgan.utils')

    utils.init_weights = lambda module: None                                  # every weight is overwritten by fill() below
    utils.get_padding = lambda kernel_size, dilation=1: (kernel_size - 1) * dilation // 2       # "same" padding of an odd kernel
    sys.modules['ref_bigvgan.utils'] = utils
    torch.manual_seed(0)
    return importlib.import_module('ref_bigvgan.bigvgan'), importlib.import_module('ref_bigvgan.env')


def seeded(ns, key, shape, uniform=False):
    """float32 values, a function of (namespace, key, shape) alone."""
    rs = np.random.RandomState(zlib.crc32(f'{SEED}|{ns}|{key}|{tuple(shape)}'.encode()))
    a = (rs.uniform(0.8, 1.2, size=shape) if uniform else rs.randn(*shape)).astype(np.float32)
    return a


def cut(a):
    return (np.ascontiguousarray(a, dtype=np.float32).view(np.uint32) & np.uint32(0xFFFF0000)).view(np.float32)


def dev(q32, q64):
    scale = float(q64.abs().max())
    return float((q32.double() - q64).abs().max()) / scale if scale > 0 else float((q32.double() - q64).abs().max())


def fill(model, ns, free_g):
    """Seeded parameters into a reference model: into ``weight_v`` / ``weight_g`` while it is weight-normed, else into ``weight``."""
    import torch
    from torch import nn
    with torch.no_grad():
        for name, m in model.named_modules():
            if isinstance(m, (nn.Conv1d, nn.ConvTranspose1d)):
                normed = hasattr(m, 'weight_v')
                target = m.weight_v if normed else m.weight
                shape = tuple(target.shape)
                fan_in = (shape[0] if isinstance(m, nn.ConvTranspose1d) else shape[1]) * shape[2]
                target.copy_(torch.from_numpy(cut(seeded(ns, name + '.weight', shape) / np.sqrt(fan_in))))
                if normed:
                    g = torch.norm_except_dim(m.weight_v, 2, 0)
                    if free_g:
                        g = g * torch.from_numpy(seeded(ns, name + '.weight_g', tuple(g.shape), uniform=True))
                    m.weight_g.copy_(g)
                if m.bias is not None:
                    m.bias.copy_(torch.from_numpy(cut(0.1 * seeded(ns, name + '.bias', tuple(m.bias.shape)))))
        for name, p in model.named_parameters():
            if name.endswith(('.alpha', '.beta')):
                p.copy_(torch.from_numpy(cut(0.3 * seeded(ns, name, tuple(p.shape)))))


def main():
    import torch
    root = sys.argv[1] if len(sys.argv) > 1 else '/root/reference'
    ref, env = load_reference(root)
    out, cases = {}, {}
    worst = [0., '']
    chunks, where, size = [], {}, [0]

    def pool(ns, state):
        """key -> [offset, shape] of every tensor of ``state`` in the pool; an array already there (same namespace, key, shape) is reused."""
        index = {}
        for key, v in state.items():
            a = v.detach().numpy()
            assert a.dtype == np.float32, (key, a.dtype)
            name = (ns, key, a.shape)
            if name in where:
                assert np.array_equal(chunks[where[name][0]], a.reshape(-1)), name
            else:
                where[name] = (len(chunks), size[0])
                chunks.append(a.reshape(-1).copy())
                size[0] += a.size
            index[key] = [where[name][1], list(a.shape)]
        return index

    def trace(model, x):
        """The output and the intermediates of ``model(x)``: ``dict(y, pre, up<i>, mean<i>)``."""
        got = {}
        hooks = [model.conv_pre.register_forward_hook(lambda m, i, o: got.__setitem__('pre', o.detach().clone()))]
        n = len(model.ups)
        for i in range(n):
            hooks.append(model.ups[i][0].register_forward_hook(lambda m, a, o, i=i: got.__setitem__(f'up{i}', o.detach().clone())))
            after = model.ups[i + 1][0] if i + 1 < n else model.activation_post
            hooks.append(after.register_forward_pre_hook(lambda m, a, i=i: got.__setitem__(f'mean{i}', a[0].detach().clone())))
        with torch.no_grad():
            got['y'] = model(x)
        for hk in hooks:
            hk.remove()
        return got

    for name, change, shape in CASES:
        h = dict(BASE, **change)
        model = ref.BigVGAN(env.AttrDict(json.loads(json.dumps(h))))
        meta = dict(h=h, shape=list(shape))
        if name == 'k1':
            fill(model, 'k1', free_g=True)
            meta['sd_wn'] = pool('k1wn', model.state_dict())
            model.remove_weight_norm()
            meta['sd'] = pool('k1', model.state_dict())
        else:
            model.remove_weight_norm()
            fill(model, 'w', free_g=False)
            meta['sd'] = pool('w', model.state_dict())
        model.eval()
        rs = np.random.RandomState(zlib.crc32(f'{SEED}|x|{name}'.encode()))
        x = torch.from_numpy((X_SCALE * rs.randn(*shape)).astype(np.float32))
        r32 = trace(model, x)
        r64 = trace(model.double(), x.double())
        out[f'{name}_x'] = x.numpy()
        for q, v in r64.items():
            assert v.dtype == torch.float64 and r32[q].dtype == torch.float32 and bool(torch.isfinite(v).all()), (name, q)
            out[f'{name}_{q}'] = v.numpy()
            d = out[f'{name}_dev32_{q}'] = dev(r32[q], v)
            if d > worst[0]:
                worst[:] = [d, f'{name}_{q}']
            assert d < DEV32_MAX, (name, q, d)
        meta['out_shape'] = list(r64['y'].shape)
        meta['quantities'] = list(r64)
        cases[name] = meta
        print(f'{name:8s} {str(list(shape)):10s} -> {str(meta["out_shape"]):12s} max|y| {float(r64["y"].abs().max()):.3f}  '
              + '  '.join(f'{q} {out[f"{name}_dev32_{q}"]:.2g}' for q in r64))
    rate = int(np.prod(BASE['upsample_rates']))
    assert cases['amp1']['out_shape'] == [2, 1, 9 * rate] and cases['pad_odd']['out_shape'] == [1, 1, 11], cases['pad_odd']['out_shape']
    out['pool'] = np.concatenate(chunks)
    out['cases'] = json.dumps(cases)
    print(f'largest dev32: {worst[0]:.3g} ({worst[1]}); pool: {out["pool"].size} values')
    path = HERE / 'g23_bigvgan.npz'
    np.savez_compressed(path, **out)
    print(path, path.stat().st_size, 'bytes')


if __name__ == '__main__':
    main()
