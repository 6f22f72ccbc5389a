#!/usr/bin/env python3
"""Generate tests/golden/g21_anti_alias.npz by running the REAL reference's torch formulation of BigVGAN's anti-aliased activation:
``nvidia_bigvgan/activations.py`` (Snake, SnakeBeta) and ``nvidia_bigvgan/alias_free_activation/torch/{filter,resample,act}.py``
(kaiser_sinc_filter1d, LowPassFilter1d, UpSample1d, DownSample1d, Activation1d).

Run where the reference tree is available (default /root/reference, or the first argument):

    python tests/golden/make_golden_anti_alias.py

How the reference is loaded: the vocoder package's ``__init__`` pulls the generator and ``huggingface_hub``, so ``nvidia_bigvgan``,
``.alias_free_activation`` and ``.alias_free_activation.torch`` are registered as EMPTY stand-in packages (under the name ``ref_bigvgan``)
whose ``__path__`` points at the real directories; the five modules imported from them are the reference's files.  They need torch only.
The output is data only.

Every case: ``x`` (seeded randn), the parameters, output-gradient weights ``w``, all float32; the reference's own float32 filters
(``up_filter``, ``down_filter``); the reference run in float64 (modules ``.double()``: the float32 filters widened, the inputs widened):
``y``, and ``dx``, ``dalpha``, ``dbeta`` of ``sum(y w)``; ``dev32_<q>``: the deviation of the reference's float32 run from that,
``max|q32 - q64| / max|q64|`` (0 where ``q64`` is all zero).  ``cases`` (json): per case the class, ``logscale``, ratios, kernel sizes, shape.

    d<T>_snake / d<T>_beta   default 2 / 2 / 12 / 12 at [2,3,1], [2,3,5], [1,4,37], [2,5,300]; Snake linear (alpha ~ 1.5 +- 0.5), SnakeBeta log
    big_*      [2,3,41], log alpha ~ 2 +- 0.3, x = 2 randn (sine arguments to ~50)
    zero_*     [2,3,41], linear alpha = (0, 1, 2.5), beta = (0, 0.5, 2)
    neglog_*   [2,3,41], log parameters ~ -6
    g331818, g2279, g42812, g111212   (up ratio, down ratio, up taps, down taps) at [2,3,11], SnakeBeta log
    up3, down2, down3 on [1,2,9], lp7 = LowPassFilter1d(stride=1, padding=False, kernel_size=7) on [1,2,20]   (x, w, filter, y, dx)
``filters`` : kaiser_sinc_filter1d for ``filter_args``; ``keys_snake`` / ``keys_snakebeta``: the state_dict keys of Activation1d.

Condition (asserted; move the seed if it fails): every ``dev32_*`` below 2e-5.
"""
import importlib
import json
import sys
import types
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
DEV32_MAX = 2e-5
FILTER_ARGS = [(0.25, 0.3, 12), (0.5 / 3, 0.2, 18), (0.125, 0.15, 8), (0.25, 0.3, 7), (0.5, 0.6, 12)]


def load_reference(root):
    base = Path(root) / 'padertorch' / 'contrib' / 'mk' / 'synthesis' / 'vocoder' / 'nvidia_bigvgan'
    for name, path in [('ref_bigvgan', base), ('ref_bigvgan.alias_free_activation', base / 'alias_free_activation'),
                       ('ref_bigvgan.alias_free_activation.torch', base / 'alias_free_activation' / 'torch')]:
        pkg = types.ModuleType(name)
        pkg.__path__ = [str(path)]
        sys.modules[name] = pkg
    mods = types.SimpleNamespace()
    mods.activations = importlib.import_module('ref_bigvgan.activations')
    mods.filter = importlib.import_module('ref_bigvgan.alias_free_activation.torch.filter')
    mods.resample = importlib.import_module('ref_bigvgan.alias_free_activation.torch.resample')
    mods.act = importlib.import_module('ref_bigvgan.alias_free_activation.torch.act')
    return mods


def dev(q32, q64):
    scale = float(q64.abs().max())
    return float((q32.double() - q64).abs().max()) / scale if scale > 0 else float((q32.double() - q64).abs().max())


def main():
    import torch
    root = sys.argv[1] if len(sys.argv) > 1 else '/root/reference'
    ref = load_reference(root)
    out, cases = {}, {}
    worst = [0., '']

    def run_module(make, x, w, dtype):
        """``make()`` -> a fresh reference module with the case's parameters set (float32); run in ``dtype``."""
        m = make()
        if dtype == torch.float64:
            m = m.double()
        xx = x.detach().clone().to(dtype).requires_grad_(True)
        y = m(xx)
        (y * w.to(dtype)).sum().backward()
        res = dict(y=y.detach(), dx=xx.grad)
        act = getattr(m, 'act', None)
        if act is not None:
            res['dalpha'] = act.alpha.grad
            if hasattr(act, 'beta'):
                res['dbeta'] = act.beta.grad
        return m, res

    def add_case(name, make, x, meta):
        y_shape = make()(x).shape
        w = torch.from_numpy(rng.randn(*y_shape).astype(np.float32))
        m32, r32 = run_module(make, x, w, torch.float32)
        m64, r64 = run_module(make, x, w, torch.float64)
        pre = name + '_'
        out[pre + 'x'], out[pre + 'w'] = x.numpy(), w.numpy()
        for q, v in r64.items():
            assert v.dtype == torch.float64 and bool(torch.isfinite(v).all()), (name, q)
            assert r32[q].dtype == torch.float32 and bool(torch.isfinite(r32[q]).all()), (name, q)
            out[pre + q] = v.numpy()
            d = out[pre + 'dev32_' + q] = dev(r32[q], v)
            if d > worst[0]:
                worst[:] = [d, pre + q]
            assert d < DEV32_MAX, (name, q, d)
        if hasattr(m32, 'act'):
            out[pre + 'alpha'] = m32.act.alpha.detach().numpy()
            if hasattr(m32.act, 'beta'):
                out[pre + 'beta'] = m32.act.beta.detach().numpy()
            out[pre + 'up_filter'] = m32.upsample.filter.numpy()
            out[pre + 'down_filter'] = m32.downsample.lowpass.filter.numpy()
            assert m32.upsample.filter.dtype == torch.float32
        else:
            f = m32.filter if hasattr(m32, 'filter') else m32.lowpass.filter
            out[pre + 'filter'] = f.numpy()
        cases[name] = dict(meta, shape=list(x.shape), out_shape=list(y_shape))
        print(f'{name:16s} {str(list(x.shape)):14s} -> {str(list(y_shape)):14s} '
              + '  '.join(f'dev32_{q} {out[pre + "dev32_" + q]:.2g}' for q in r64))

    def activation(cls, logscale, alpha, beta=None, geometry=(2, 2, 12, 12)):
        def make():
            act = getattr(ref.activations, cls)(len(alpha), alpha_logscale=logscale)
            with torch.no_grad():
                act.alpha.copy_(torch.from_numpy(np.asarray(alpha, dtype=np.float32)))
                if cls == 'SnakeBeta':
                    act.beta.copy_(torch.from_numpy(np.asarray(beta, dtype=np.float32)))
            r, d, k, dk = geometry
            return ref.act.Activation1d(act, up_ratio=r, down_ratio=d, up_kernel_size=k, down_kernel_size=dk)
        return make

    def meta(cls, logscale, geometry=(2, 2, 12, 12)):
        r, d, k, dk = geometry
        return dict(cls=cls, logscale=logscale, up_ratio=r, down_ratio=d, up_kernel_size=k, down_kernel_size=dk)

    rng = np.random.RandomState(2100)
    for shape in [(2, 3, 1), (2, 3, 5), (1, 4, 37), (2, 5, 300)]:
        C = shape[1]
        x = torch.from_numpy(rng.randn(*shape).astype(np.float32))
        add_case(f'd{shape[2]}_snake', activation('Snake', False, 1.5 + 0.5 * rng.randn(C)), x, meta('Snake', False))
        add_case(f'd{shape[2]}_beta', activation('SnakeBeta', True, 0.5 * rng.randn(C), 0.5 * rng.randn(C)), x, meta('SnakeBeta', True))
    shape = (2, 3, 41)
    x = torch.from_numpy((2 * rng.randn(*shape)).astype(np.float32))
    add_case('big_snake', activation('Snake', True, 2 + 0.3 * rng.randn(3)), x, meta('Snake', True))
    add_case('big_beta', activation('SnakeBeta', True, 2 + 0.3 * rng.randn(3), 2 + 0.3 * rng.randn(3)), x, meta('SnakeBeta', True))
    x = torch.from_numpy(rng.randn(*shape).astype(np.float32))
    add_case('zero_snake', activation('Snake', False, [0., 1., 2.5]), x, meta('Snake', False))
    add_case('zero_beta', activation('SnakeBeta', False, [0., 1., 2.5], [0., 0.5, 2.]), x, meta('SnakeBeta', False))
    add_case('neglog_snake', activation('Snake', True, -6 + 0.1 * rng.randn(3)), x, meta('Snake', True))
    add_case('neglog_beta', activation('SnakeBeta', True, -6 + 0.1 * rng.randn(3), -6 + 0.1 * rng.randn(3)), x, meta('SnakeBeta', True))
    for geometry in [(3, 3, 18, 18), (2, 2, 7, 9), (4, 2, 8, 12), (1, 1, 12, 12)]:
        x = torch.from_numpy(rng.randn(2, 3, 11).astype(np.float32))
        name = 'g' + ''.join(str(v) for v in geometry)
        add_case(name, activation('SnakeBeta', True, 0.5 * rng.randn(3), 0.5 * rng.randn(3), geometry), x, meta('SnakeBeta', True, geometry))
    assert cases['g42812']['out_shape'] == [2, 3, 22]
    x = torch.from_numpy(rng.randn(1, 2, 9).astype(np.float32))
    add_case('up3', lambda: ref.resample.UpSample1d(3), x, dict(cls='UpSample1d', ratio=3))
    add_case('down2', lambda: ref.resample.DownSample1d(2), x, dict(cls='DownSample1d', ratio=2))
    add_case('down3', lambda: ref.resample.DownSample1d(3), x, dict(cls='DownSample1d', ratio=3))
    x = torch.from_numpy(rng.randn(1, 2, 20).astype(np.float32))
    add_case('lp7', lambda: ref.filter.LowPassFilter1d(stride=1, padding=False, kernel_size=7), x,
             dict(cls='LowPassFilter1d', stride=1, padding=False, kernel_size=7))

    for i, args in enumerate(FILTER_ARGS):
        f = ref.filter.kaiser_sinc_filter1d(*args)
        assert f.dtype == torch.float32 and tuple(f.shape) == (1, 1, args[2])
        out[f'filters_{i}'] = f.numpy()
    out['filter_args'] = np.array(FILTER_ARGS, dtype=np.float64)
    out['keys_snake'] = json.dumps(list(ref.act.Activation1d(ref.activations.Snake(3)).state_dict()))
    out['keys_snakebeta'] = json.dumps(list(ref.act.Activation1d(ref.activations.SnakeBeta(3)).state_dict()))
    out['cases'] = json.dumps(cases)
    print(f'largest dev32: {worst[0]:.3g} ({worst[1]})')
    path = HERE / 'g21_anti_alias.npz'
    np.savez_compressed(path, **out)
    print(path, path.stat().st_size, 'bytes')


if __name__ == '__main__':
    main()
