#!/usr/bin/env python3
"""Generate tests/golden/g20_griffin_lim.npz by running the REAL reference's fast Griffin-Lim
(padertorch/contrib/mk/synthesis/parametric/griffin_lim.py: ``griffin_lim_step``, ``fast_griffin_lim``) on its own ``padertorch.ops.STFT``.

Run where the reference tree is available (default /root/reference, or the first argument):

    python tests/golden/make_golden_griffin_lim.py

How the reference is loaded: ``ref_shim``, the repository and the reference go on ``sys.path`` as in make_golden_orpit.py.  The
``synthesis`` package's ``__init__`` pulls the neural vocoders, so ``padertorch.contrib.mk``, ``.synthesis`` and ``.parametric`` are
registered as EMPTY stand-in packages whose ``__path__`` points at the real directories; ``griffin_lim.py`` and ``base.py`` are then the
reference's files.  ``paderbox.transform.STFT`` and ``paderbox.transform.module_resample.resample_sox`` (absent from the shim; only
imported, never called here) are set to stand-ins inside this recipe.  The output is data only.

Cases (``a = |STFT(randn)|`` of a seeded float64 signal, ``x0 = a exp(j U[-pi, pi))`` as complex64, alpha 0.95):

    s64    size 64, shift 16, blackman, fading 'full', 2 rows, 28 frames   (3 work items of 8 frames plus a partial one)
    s512   512 / 128, blackman, 1 row, 19 frames                           (4 items of 4 plus 3)
    s40    size 40, shift 10, hann, 3 rows, 13 frames                      (direct-DFT path)
    s512w  512 / 20, window_length 40, hamming, 1 row, 16 frames           (the reference's third test geometry)

The fp32 run is ``fast_griffin_lim(a32, stft, atol=0, x=x0)`` of the reference; the fp64 run is the same loop through the reference's
``griffin_lim_step`` on float64 ``a`` and complex128 ``y`` (the entry point refuses a complex128 ``x``).  The recipe asserts that this
loop, run in fp32, and the entry point give IDENTICAL signals.

Keys per case ``<c>_``: ``a`` (float32), ``x0`` (complex64), ``x64_1`` .. ``x64_3`` (complex128: ``x`` behind iteration n), ``dev32_1`` ..
``dev32_3``, ``dev32_30`` (``max|x32_n - x64_n| / max(a)``), ``rmse64`` / ``rmse32`` [30], ``sig64_3`` / ``sig64_30``, ``devsig32_3`` /
``devsig32_30`` (``max|sig32 - sig64| / max|sig64|``), ``seed``; ``geometries`` (json): the STFT arguments and shapes.
``edge_``: one ``griffin_lim_step`` at size 64 / 16 with ``a`` exactly 0 in some bins, ``y`` exactly 0 in others (where ``a > 0``) and
``y = 1e-25 (1 + 1j)`` in others: ``a``, ``y`` (complex64), ``idx_a0`` / ``idx_y0`` / ``idx_tiny`` (flat indices), ``P64``, ``audio64``, ``x64``.
``stop_``: on s64, ``atol`` = the geometric mean of ``rmse64[k-1]`` and ``rmse64[k]`` for the first k in 8..16 with a margin of 1e-3
(every ``rmse64`` before k above ``atol (1 + 1e-3)``, ``rmse64[k]`` below ``atol (1 - 1e-3)``): ``atol``, ``k``, ``sig64`` (stopped behind
k + 1 iterations).  The RMSE is not monotone (iteration 2 lies above iteration 1).
``grad0_``: on s64, ``iterations=0`` (lines 151-155, the phase of ``x0`` taken in fp64): ``sig64``, ``w`` and ``grad64 = d sum(signal * w) / d a``.

Conditions (enforced by moving the seed, asserted at the end): ``rmse32`` within 5e-5 relative of ``rmse64`` at every iteration of
every case.
"""
import importlib
import json
import sys
import types
from pathlib import Path

HERE = Path(__file__).resolve().parent
REPO = HERE.parent.parent

import numpy as np  # noqa: E402

ALPHA = 0.95
ITERATIONS = 30
RMSE_REL = 5e-5
CASES = {
    's64': dict(seed=2001, rows=2, samples=400, frames=28, stft=dict(size=64, shift=16, window='blackman', fading='full')),
    's512': dict(seed=2002, rows=1, samples=2048, frames=19, stft=dict(size=512, shift=128, window='blackman', fading='full')),
    's40': dict(seed=2003, rows=3, samples=100, frames=13, stft=dict(size=40, shift=10, window='hann', fading='full')),
    's512w': dict(seed=2004, rows=1, samples=300, frames=16,
                  stft=dict(size=512, shift=20, window_length=40, window='hamming', fading='full')),
}


def load_reference(root):
    sys.path[:0] = [str(HERE / 'ref_shim'), str(REPO), root]
    import paderbox.transform
    paderbox.transform.STFT = type('STFT', (), {})                       # imported for isinstance checks only
    resample = types.ModuleType('paderbox.transform.module_resample')
    resample.resample_sox = None                                         # imported by base.py, never called here
    sys.modules['paderbox.transform.module_resample'] = resample
    paderbox.transform.module_resample = resample
    import padertorch  # noqa: F401
    base = Path(root) / 'padertorch' / 'contrib' / 'mk'
    for name, path in [('padertorch.contrib.mk', base), ('padertorch.contrib.mk.synthesis', base / 'synthesis'),
                       ('padertorch.contrib.mk.synthesis.parametric', base / 'synthesis' / 'parametric')]:
        pkg = types.ModuleType(name)
        pkg.__path__ = [str(path)]
        sys.modules[name] = pkg
    return importlib.import_module('padertorch.contrib.mk.synthesis.parametric.griffin_lim')


def loop(gl, a, x0, stft, iterations, atol=0.):
    """The loop of fast_griffin_lim (lines 132-155) through the reference's griffin_lim_step, in the dtype of ``a``; returns the ``x`` behind
    every iteration, the RMSEs and the signal."""
    import torch
    cdtype = torch.complex128 if a.dtype == torch.float64 else torch.complex64
    with torch.no_grad():
        x = a * torch.exp(1.0j * torch.angle(x0.to(cdtype)))
        y = x
        xs, rmse = [], []
        for _ in range(iterations):
            x_, _audio = gl.griffin_lim_step(a, y, stft)
            y = x_ + ALPHA * (x_ - x)
            x = x_
            xs.append(x)
            rmse.append(float(torch.sqrt(torch.mean((torch.abs(x) - a) ** 2))))
            if rmse[-1] < atol:
                break
        signal = stft.inverse(a * torch.exp(1.0j * torch.angle(x)))
    return xs, np.array(rmse), signal


def main():
    import torch
    root = sys.argv[1] if len(sys.argv) > 1 else '/root/reference'
    gl = load_reference(root)
    from padertorch.ops import STFT
    out, geometries = {}, {}
    for name, case in CASES.items():
        rng = np.random.RandomState(case['seed'])
        stft = STFT(**case['stft'])
        sig = torch.from_numpy(rng.randn(case['rows'], case['samples']))
        a64 = torch.abs(stft(sig))
        assert a64.dtype == torch.float64 and a64.shape[-2] == case['frames'], (a64.dtype, a64.shape)
        a32 = a64.to(torch.float32)
        a64 = a32.to(torch.float64)                    # both runs start from the SAME (float32-representable) magnitudes
        phase = rng.uniform(-np.pi, np.pi, size=tuple(a64.shape))
        x0 = (a64 * torch.exp(1.0j * torch.from_numpy(phase))).to(torch.complex64)
        xs64, rmse64, sig64_30 = loop(gl, a64, x0, stft, ITERATIONS)
        xs32, rmse32, sig32_30 = loop(gl, a32, x0, stft, ITERATIONS)
        _, _, sig64_3 = loop(gl, a64, x0, stft, 3)
        _, _, sig32_3 = loop(gl, a32, x0, stft, 3)
        for its, mine in [(3, sig32_3), (ITERATIONS, sig32_30)]:
            entry = gl.fast_griffin_lim(a32, stft, alpha=ALPHA, iterations=its, atol=0, x=x0)
            assert entry.dtype == torch.float32 and torch.equal(entry, mine), (name, its)
        amax = float(a64.max())
        pre = name + '_'
        out[pre + 'a'], out[pre + 'x0'], out[pre + 'seed'] = a32.numpy(), x0.numpy(), case['seed']
        for n in (1, 2, 3):
            out[pre + f'x64_{n}'] = xs64[n - 1].numpy()
        for n in (1, 2, 3, ITERATIONS):
            out[pre + f'dev32_{n}'] = float((xs32[n - 1].to(torch.complex128) - xs64[n - 1]).abs().max()) / amax
        out[pre + 'rmse64'], out[pre + 'rmse32'] = rmse64, rmse32
        for n, s64, s32 in [(3, sig64_3, sig32_3), (ITERATIONS, sig64_30, sig32_30)]:
            out[pre + f'sig64_{n}'] = s64.numpy()
            out[pre + f'devsig32_{n}'] = float((s32.to(torch.float64) - s64).abs().max() / s64.abs().max())
        rel = float(np.max(np.abs(rmse32 - rmse64) / rmse64))
        print(f'{name}: frames {a64.shape[-2]}  rmse64 {rmse64[0]:.4g} {rmse64[1]:.4g} {rmse64[2]:.4g} .. {rmse64[-1]:.4g}  rmse32 rel {rel:.2g}  '
              + '  '.join(f'dev32_{n} {out[pre + f"dev32_{n}"]:.2g}' for n in (1, 2, 3, ITERATIONS))
              + f'  devsig32 {out[pre + "devsig32_3"]:.2g} {out[pre + "devsig32_30"]:.2g}')
        assert rel < RMSE_REL, (name, rel)
        geometries[name] = dict(case['stft'], rows=case['rows'], frames=case['frames'], samples=int(sig64_30.shape[-1]))

        if name == 's64':
            # stop case
            k = None
            for cand in range(8, 17):
                atol = float(np.sqrt(rmse64[cand - 1] * rmse64[cand]))
                if np.all(rmse64[:cand] > atol * (1 + 1e-3)) and rmse64[cand] < atol * (1 - 1e-3):
                    k = cand
                    break
            assert k is not None, rmse64
            xs, r, sig = loop(gl, a64, x0, stft, ITERATIONS, atol=atol)
            assert len(r) == k + 1, (len(r), k)
            assert not np.all(np.diff(rmse64) < 0), 'the RMSE is expected not to be monotone'
            out['stop_atol'], out['stop_k'], out['stop_sig64'] = atol, k, sig.numpy()
            # grad0
            w = rng.randn(*sig64_30.shape)
            aw = a64.clone().requires_grad_(True)
            # lines 151-155 with the phase in fp64 (the entry point takes the angle of the complex64 x0 in fp32: 5e-8 away)
            s0 = stft.inverse(aw * torch.exp(1.0j * torch.angle(x0.to(torch.complex128))))
            entry = gl.fast_griffin_lim(aw, stft, alpha=ALPHA, iterations=0, atol=0, x=x0)
            assert s0.dtype == torch.float64 and float((entry - s0).abs().max() / s0.abs().max()) < 1e-6
            (s0 * torch.from_numpy(w)).sum().backward()
            out['grad0_w'], out['grad0_grad64'], out['grad0_sig64'] = w, aw.grad.numpy(), s0.detach().numpy()

    # edge: one step with exact zeros and tiny bins
    rng = np.random.RandomState(2010)
    stft = STFT(size=64, shift=16, window='blackman', fading='full')
    a = np.abs(rng.randn(2, 12, 33)).astype(np.float32) + 0.1
    y = (rng.randn(2, 12, 33) + 1j * rng.randn(2, 12, 33)).astype(np.complex64)
    idx = rng.permutation(a.size)
    idx_a0, idx_y0, idx_tiny = np.sort(idx[:40]), np.sort(idx[40:80]), np.sort(idx[80:120])
    a.reshape(-1)[idx_a0] = 0.
    y.reshape(-1)[idx_y0] = 0.
    y.reshape(-1)[idx_tiny] = np.complex64(1e-25 * (1 + 1j))
    a64, y64 = torch.from_numpy(a.astype(np.float64)), torch.from_numpy(y.astype(np.complex128))
    P64 = a64 * torch.exp(1.0j * torch.angle(y64))
    x64, audio64 = gl.griffin_lim_step(a64, y64, stft)
    assert x64.dtype == torch.complex128 and x64.shape == a64.shape
    want = a.astype(np.float64).reshape(-1)
    assert np.all(P64.numpy().reshape(-1)[idx_y0] == want[idx_y0]) and np.all(P64.numpy().reshape(-1)[idx_a0] == 0)
    assert np.allclose(P64.numpy().reshape(-1)[idx_tiny], want[idx_tiny] * np.sqrt(0.5) * (1 + 1j), rtol=1e-12)
    out.update(edge_a=a, edge_y=y, edge_idx_a0=idx_a0, edge_idx_y0=idx_y0, edge_idx_tiny=idx_tiny, edge_P64=P64.numpy(),
               edge_audio64=audio64.numpy(), edge_x64=x64.numpy())
    geometries['edge'] = dict(size=64, shift=16, window='blackman', fading='full', rows=2, frames=12, samples=int(audio64.shape[-1]))

    out['geometries'] = json.dumps(geometries)
    out['alpha'], out['iterations'] = ALPHA, ITERATIONS
    path = HERE / 'g20_griffin_lim.npz'
    np.savez_compressed(path, **out)
    print(path, path.stat().st_size, 'bytes')


if __name__ == '__main__':
    main()
