#!/usr/bin/env python3
"""Generate tests/golden/g28_je_conv_transpose.npz by importing the REAL reference's transposed convolution stack
(padertorch/contrib/je/modules/conv.py, conv_utils.py).

Run in the build container only (needs /root/reference and einops):

    python tests/golden/make_golden_je_conv_transpose.py

The pattern is make_golden_je_conv2d.py's; ``shares`` and ``store`` are make_golden_je_conv.py's.  The output is data only: parameters and
the results of an fp64 and an fp32 run of the reference.  Inputs are NOT stored: ``inputs`` draws them from a seeded numpy RandomState and
the tests call the same function.  A case is an autoencoder: a ``CNN1d`` / ``CNN2d`` (``CASES``: stride 2 first, batch norm, a residual
connection around the last layer, a max pool with indices behind it) and the ``CNNTranspose1d`` / ``CNNTranspose2d`` the reference's own
``get_transpose_config`` mirrors from it, called as

    h, lengths, indices = encoder(x, LENGTHS)
    y, lengths = decoder(h, lengths, target_shape=x.shape, target_sequence_lengths=LENGTHS, pool_indices=indices)

with the functional ``sum(y * r)``; biases, ``gamma`` and ``beta`` carry a seeded perturbation of 0.3 N(0, 1).  Keys per case: ``_keys``
(the state dict of ``ModuleList([encoder, decoder])``), ``_names``, ``_p_<key>``, ``_y64`` / ``_y32``, ``_g64_<name>`` / ``_g32_<name>``
(``x``: the input), ``_len``, ``_idx`` (the pool's indices), ``_mirror`` (the mirrored config as JSON, the factory by name).

The reference's own fp32 run must stay within a QUARTER of every gate; the generator prints the shares and refuses to write otherwise.
"""
import importlib.util
import json
import sys
from pathlib import Path

HERE = Path(__file__).resolve().parent
REPO = HERE.parent.parent

import numpy as np  # noqa: E402

_spec = importlib.util.spec_from_file_location('make_golden_je_conv', HERE / 'make_golden_je_conv.py')
g26 = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(g26)

LENGTHS = [20, 11]
SHARE = 0.25
#: name -> (encoder class name, its config, input shape)
CONFIG = dict(in_channels=3, out_channels=[8, 8, 8], kernel_size=3, stride=[2, 1, 1], pool_size=[1, 1, 2], residual_connections=[None, 3, None],
              pad_type='both', norm='batch', return_pool_indices=True)
CASES = {'t1': ('CNN1d', CONFIG, (2, 3, 20)), 't2': ('CNN2d', CONFIG, (2, 3, 12, 20))}


def seed_of(case):
    return 2800 + sorted(CASES).index(case)


def inputs(case, out_shape=None):
    """``x`` float32 and, with ``out_shape``, ``r``."""
    rng = np.random.RandomState(seed_of(case))
    x = rng.randn(*CASES[case][2]).astype(np.float32)
    return x if out_shape is None else (x, rng.randn(*out_shape).astype(np.float32))


def build(case, mods, mirror, dtype):
    """``ModuleList([encoder, decoder])`` of ``case`` from the classes ``mods`` (name -> class) and the function ``mirror`` (config with
    a ``factory`` -> mirrored config), with seeded, perturbed parameters."""
    import torch
    cls, config, _ = CASES[case]
    torch.manual_seed(seed_of(case))
    transposed = mirror(dict(config, factory=mods[cls], out_channels=list(config['out_channels'])))
    factory = transposed.pop('factory')
    net = torch.nn.ModuleList([mods[cls](**config), factory(**transposed)])
    rng = np.random.RandomState(100 + seed_of(case))
    with torch.no_grad():
        for name, p in net.named_parameters():
            if name.endswith(('bias', 'gamma', 'beta')):
                p.add_(torch.from_numpy(0.3 * rng.randn(*p.shape)).to(p.dtype))
    return net.to(dtype), dict(transposed, factory=factory.__name__)


def call(net, x):
    """``(y, lengths, pool indices)`` of the autoencoder."""
    h, lengths, indices = net[0](x, list(LENGTHS))
    y, lengths = net[1](h, lengths, target_shape=tuple(x.shape), target_sequence_lengths=list(LENGTHS), pool_indices=indices)
    return y, lengths, indices


def run(case, mods, mirror, dtype):
    import torch
    net, transposed = build(case, mods, mirror, dtype)
    x = torch.from_numpy(inputs(case)).to(dtype).requires_grad_()
    y, lengths, indices = call(net, x)
    assert y.shape == x.shape, (y.shape, x.shape)
    r0 = inputs(case, tuple(y.shape))[1]
    named = list(net.named_parameters())
    grads = torch.autograd.grad((y * torch.from_numpy(r0).to(dtype)).sum(), [x] + [p for _, p in named])
    res = {'y': y.detach().numpy().copy(), 'g_x': grads[0].numpy().copy(), 'len': np.asarray(lengths), 'idx': indices[-1].numpy().copy()}
    for (n, _), g in zip(named, grads[1:]):
        res['g_' + n] = g.numpy().copy()
    return res, net, transposed


def main():
    sys.path[:0] = [str(HERE / 'ref_shim'), str(REPO), '/root/reference']
    if not hasattr(np, 'int'):
        np.int = int
    import torch
    from padertorch.contrib.je.modules import conv as ref_conv  # the reference

    torch.set_num_threads(1)
    # (warn only: the CPU max unpooling declares no deterministic form; with a stride equal to the size no two windows share a position)
    torch.use_deterministic_algorithms(True, warn_only=True)
    mods = {'CNN1d': ref_conv.CNN1d, 'CNN2d': ref_conv.CNN2d}

    def mirror(config):
        return config['factory'].get_transpose_config(config)
    out, worst = {}, 0.
    for case in CASES:
        r64, _, transposed = run(case, mods, mirror, torch.float64)
        r32, net32, _ = run(case, mods, mirror, torch.float32)
        sh = g26.shares(r32, r64)
        state = build(case, mods, mirror, torch.float32)[0].state_dict()
        out[case + '_keys'] = np.array(json.dumps(list(state)))
        out[case + '_names'] = np.array(json.dumps([n for n, _ in net32.named_parameters()]))
        out[case + '_mirror'] = np.array(json.dumps(transposed))
        for k, v in state.items():
            out[f'{case}_p_{k}'] = v.numpy().copy()
        g26.store(out, case + '_', r64, r32)
        print(case, 'worst share %.3f (%s)' % (max(sh.values()), max(sh, key=sh.get)))
        worst = max(worst, max(sh.values()))
    assert worst <= SHARE, f'the reference\'s fp32 run is {worst:.3f} of a gate from its fp64 run (limit {SHARE})'
    path = HERE / 'g28_je_conv_transpose.npz'
    np.savez_compressed(path, **out)
    print(path, path.stat().st_size, 'bytes; worst share %.3f' % worst)


if __name__ == '__main__':
    main()
