"""STFT / iSTFT / PIT-feature / (log-)mel kernels (``csrc/stft.hip``) per ROW AND FRAME against the fp64 oracle (GPU).

The gate is ``oracle/stft_fp32.py``: ``r[b, t] = max_k |got - want| / ||want[b, t, :]||_2`` (frames that are exactly zero in the oracle
must be exactly zero), held against ``MARGIN`` times the same figure ``r32`` of an fp32 restatement on the CPU (``torch.fft`` on
float32) - so the small frames with load paths of their own (fading, the clamped / patched last frame of an odd-length row, rows of a
ragged batch with live data behind their end) count like every other frame.  ``tests/test_spectral_gate_host.py`` shows on the host
what this gate catches and the whole-tensor gate of ``tests/test_gpu_stft.py`` does not.

Shapes: B = 3 rows of N = 5 * size + 17 samples (odd), ``standard_normal``; every FFT plan (64 .. 2048), the direct-DFT sizes 100
and 6, and at sizes 64 and 512 the options that select other load paths.  The rows of an ``[B, N]`` batch with ``N`` odd have an odd
stride and take the 4-byte loads only: buffers of ``N + 1`` columns (every plan, and the ragged cases) drive the 8-byte loads (the
prefetched interior frames, the clamped edge frames, the separately fetched last sample).  The mel kernels' bounds are derived, not measured
(non-negative products: ``(8 cnt[m] + 2) 2^-24`` relative per filter of ``cnt[m]`` 8-bin groups).

Measured on an MI355X (``max r / max r32``, the worst case of each kernel; every case prints its own); ``MARGIN`` stays 8:
    forward      2.31  (direct DFT, size 100; FFT plans: 1.44 at 64/16 without fading)
    inverse      2.61  (64/16; direct DFT 100/25: 1.67; ragged ``row_frames``: 1.26)
    features     2.61  (direct DFT, size 100, ``X_abs``; FFT plans: 1.41 at 2048; the weighted cosine: 1.11)
    fused mel    1.48  (64/16 with a hann window of 50 samples and 256/64 ragged, power 1; log outputs: 0.38 of their bound at most)
    mel_apply    0.48 of the derived bound at most
    several items per wavefront (section 8: 64/16, 4 ragged rows of 655 377 samples, 20 484 work items):
        forward 1.17;  features (K = 1) 1.23 (``X_abs``; ``Y_abs`` 1.11, the weighted cosine 0.38);  fused mel 1.08 (power 1; log
        outputs 0.34 of their bound);  one fused Griffin-Lim step against the composed path: 0 of its gate (bit-identical ``x``)
The one thing these tests found beside the 2048-point plan that never ran (its 92 KB of LDS needed the opt-in the launcher now
makes): the device ``logf`` is not correctly rounded, see :func:`_log_eps`.
"""
import functools
import os

import numpy as np
import pytest
import torch

from oracle import features_np, stft_np
from oracle import stft_fp32 as G

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
PLANS = [64, 128, 256, 512, 1024, 2048]
BASE = dict(window='blackman', window_length=None, fading='full', pad=True)


def _dev(a):
    """A device copy (the shared cases are read-only)."""
    return torch.tensor(a, device=DEV)


def _kw(**over):
    kw = dict(BASE)
    kw.update(over)
    return kw


def _options(size):
    """name -> (shift, STFT keyword arguments): what selects another load path at this size."""
    s4 = size // 4
    return {
        'half': (s4, _kw(fading='half')),
        'nofade': (s4, _kw(fading=None)),
        'nopad': (s4, _kw(pad=False)),
        'hann0.8': (s4, _kw(window='hann', window_length=int(0.8 * size))),              # 51 / 409
        'hann0.8even': (s4, _kw(window='hann', window_length=2 * int(0.4 * size))),      # 50 / 408: float2 loads under a short window
        'oddshift': (s4 + 1, _kw()),                                                    # aligned2 false
        'oddpadleft': (s4, _kw(window_length=size - 1)),                                # window_length - shift odd
    }


def _shift(size):
    return max(size // 4, 2) if size != 6 else 2


def _stft(size, shift, kw, **more):
    from padertorch_amd.ops import STFT
    return STFT(size, shift, window=kw['window'], window_length=kw['window_length'], fading=kw['fading'], pad=kw['pad'], **more)


@functools.lru_cache(maxsize=None)
def _case(size, shift, opt=None, B=3):
    """(x float32 [B, N], keyword arguments, want complex128, ref32 complex64): computed once, shared, never written to."""
    kw = _options(size)[opt][1] if opt else _kw()
    rng = np.random.RandomState(size + 7 * shift)
    x = rng.standard_normal((B, 5 * size + 17)).astype(np.float32)
    want = stft_np.stft(x, size, shift, **kw)
    ref32 = G.stft32(x, size, shift, **kw)
    for a in (x, want, ref32):
        a.setflags(write=False)
    return x, kw, want, ref32


def _ragged_lengths(size, shift, N):
    return [N, N - 1, size + 1, size, size - 1, shift + 2, 1]


def _ragged_rows(fn, x, lens, T, tail_shape, dtype):
    """``fn(x[b, :n])`` per row, zero-filled to ``T`` frames."""
    out = np.zeros((len(lens), T) + tail_shape, dtype)
    for b, n in enumerate(lens):
        v = fn(x[b, :n])
        out[b, :v.shape[0]] = v
    return out


# ------------------------------------------------------------------------------------------------ 3. forward
@pytest.mark.parametrize('size', PLANS + [100, 6])
def test_forward_every_plan_and_the_direct_dft(size):
    shift = _shift(size)
    x, kw, want, ref32 = _case(size, shift)
    xd = _dev(x)
    X = _stft(size, shift, kw)(xd)
    assert X.dtype == torch.complex64 and tuple(X.shape) == want.shape
    G.check(X.cpu().numpy(), want, ref32, f'forward {size}/{shift} complex')
    S = _stft(size, shift, kw, complex_representation='stacked')(xd)
    assert tuple(S.shape) == want.shape + (2,)
    S = S.cpu().numpy()
    G.check(S[..., 0] + 1j * S[..., 1], want, ref32, f'forward {size}/{shift} stacked')


def test_size_2048_forward_runs_its_plan():
    """Plain ``STFT(2048)`` takes the 32 x 32 plan (92 KB of LDS: the launcher opts in), not the O(size^2) direct-DFT kernel: the plan
    kernels' FFT ablation switch changes the result, the direct-DFT kernel has no such switch."""
    x, kw, want, _ = _case(2048, 512)
    xd = _dev(x)
    st = _stft(2048, 512, kw)
    X = st(xd)
    before = os.environ.get('PTMI_STFT_DBG')
    os.environ['PTMI_STFT_DBG'] = '2'
    try:
        Y = st(xd)
        torch.cuda.synchronize()
    finally:
        if before is None:
            del os.environ['PTMI_STFT_DBG']
        else:
            os.environ['PTMI_STFT_DBG'] = before
    assert not torch.equal(X, Y)
    assert torch.equal(X, st(xd))


@pytest.mark.parametrize('size', [64, 512])
@pytest.mark.parametrize('opt', list(_options(64)))
def test_forward_load_path_options(size, opt):
    shift = _options(size)[opt][0]
    x, kw, want, ref32 = _case(size, shift, opt)
    X = _stft(size, shift, kw)(_dev(x))
    assert tuple(X.shape) == want.shape
    G.check(X.cpu().numpy(), want, ref32, f'forward {size}/{shift} {opt}')


def _misaligned_row(x_row):
    """``x_row`` (odd length N) as the first N of the N + 1 samples of a device view that starts 4 bytes into an 8-byte aligned buffer,
    NaN behind it: an even stride, so that the POINTER is all that keeps the kernel from its 8-byte loads."""
    N = x_row.shape[0]
    buf = torch.full((N + 2,), float('nan'), device=DEV)
    buf[1:N + 1] = _dev(x_row)
    v = buf[1:]
    assert N % 2 == 1 and v.shape[0] == N + 1 and v.data_ptr() % 8 == 4 and v.is_contiguous()
    return v


@pytest.mark.parametrize('size', [64, 512])
def test_forward_from_a_pointer_that_is_not_8_byte_aligned(size):
    shift = size // 4
    x, kw, want, ref32 = _case(size, shift)
    v = _misaligned_row(x[1])
    X = _stft(size, shift, kw)(v, num_samples=torch.tensor([x.shape[1]], dtype=torch.int32, device=DEV)).cpu().numpy()
    T = want.shape[1]
    assert X.ndim == 2 and X.shape[0] >= T and (X[T:] == 0).all()
    G.check(X[:T], want[1], ref32[1], f'forward {size}/{shift} misaligned 1-D')


@pytest.mark.parametrize('size', PLANS)
def test_forward_odd_length_rows_at_an_even_stride(size):
    """Every plan's 8-byte load paths (interior frames prefetched, edge frames clamped, the last sample of an odd-length row fetched
    on its own): the base case's rows in a buffer of ``N + 1`` columns, NaN in the spare one.  A row stride of ``N`` (odd) - any
    ``[B, N]`` or 1-D input of the base length - selects the 4-byte loads."""
    shift = size // 4
    x, kw, want, ref32 = _case(size, shift)
    B, N = x.shape
    buf = np.full((B, N + 1), np.nan, np.float32)
    buf[:, :N] = x
    T = stft_np.num_frames(N + 1, size, shift, 'full', True)
    assert T >= want.shape[1]
    w, r = np.zeros((B, T, want.shape[2]), np.complex128), np.zeros((B, T, want.shape[2]), np.complex64)
    w[:, :want.shape[1]], r[:, :want.shape[1]] = want, ref32
    v = _dev(buf)
    assert v.data_ptr() % 8 == 0 and v.stride(0) % 2 == 0 and N % 2 == 1
    X = _stft(size, shift, kw)(v, num_samples=torch.full((B,), N, dtype=torch.int32, device=DEV))
    G.check(X.cpu().numpy(), w, r, f'forward {size}/{shift} even stride')


@pytest.mark.parametrize('size', [64, 512])
@pytest.mark.parametrize('fill', [float('nan'), 1e30])
@pytest.mark.parametrize('width', [0, 1])
def test_forward_ragged_rows_with_live_padding(size, fill, width):
    """``width`` = 1: the buffer is one column wider than the longest row, so its row stride is even and the rows take the 8-byte
    loads (with the separately fetched last sample of the odd-length ones); an ``[B, N]`` buffer with ``N`` odd never does."""
    shift = size // 4
    kw = _kw()
    N = 5 * size + 17
    lens = _ragged_lengths(size, shift, N)
    x = np.random.RandomState(size + 1).standard_normal((len(lens), N + width)).astype(np.float32)
    xf = x.copy()
    for b, n in enumerate(lens):
        xf[b, n:] = fill
    T = stft_np.num_frames(N + width, size, shift, 'full', True)
    F = size // 2 + 1
    want = _ragged_rows(lambda r: stft_np.stft(r, size, shift, **kw), x, lens, T, (F,), np.complex128)
    ref32 = _ragged_rows(lambda r: G.stft32(r, size, shift, **kw), x, lens, T, (F,), np.complex64)
    ns = torch.tensor(lens, dtype=torch.int32, device=DEV)
    X = _stft(size, shift, kw)(_dev(xf), num_samples=ns).cpu().numpy()
    assert X.shape == want.shape
    assert not np.isnan(X).any()
    for b, n in enumerate(lens):
        assert (X[b, stft_np.num_frames(n, size, shift, 'full', True):] == 0).all(), b
    G.check(X, want, ref32, f'forward {size}/{shift} ragged fill {fill} width N+{width}')


# ------------------------------------------------------------------------------------------------ 4. inverse
@pytest.mark.parametrize('size', PLANS + [100])
def test_inverse_every_plan_and_the_direct_dft(size):
    shift = _shift(size)
    x, kw, want, _ = _case(size, shift)
    Xc = want.astype(np.complex64)
    wi = stft_np.istft(Xc.astype(np.complex128), size, shift)
    ri = G.istft32(Xc, size, shift)
    got = _stft(size, shift, kw).inverse(_dev(Xc)).cpu().numpy()
    assert got.shape == wi.shape
    G.check(G.blocks_of(got, shift), G.blocks_of(wi, shift), G.blocks_of(ri, shift), f'inverse {size}/{shift}')


def test_inverse_ragged_row_frames_with_garbage_behind():
    from padertorch_amd import _lib
    size, shift = 512, 128
    x, kw, want, _ = _case(size, shift, None, 5)
    B, T, F = want.shape
    counts = [T, T - 1, 5, 1, 0]
    Xc = want.astype(np.complex64)
    clean, dirty = Xc.copy(), Xc.copy()
    for b, c in enumerate(counts):
        clean[b, c:] = 0
        dirty[b, c:] = 1e30 * (1 + 1j)
    wi = stft_np.istft(clean.astype(np.complex128), size, shift)
    ri = G.istft32(clean, size, shift)
    st = _stft(size, shift, kw)
    dev = torch.device(DEV)
    lib, tb = _lib.load(), st._tables.get(dev)
    spec = torch.view_as_real(_dev(dirty)).contiguous()
    rf = torch.tensor(counts, dtype=torch.int32, device=dev)
    n = int(lib.ptmi_istft_num_samples(st._geom, T))
    assert n == wi.shape[-1]
    out = torch.full((B, n), float('nan'), device=dev)
    _lib.check(lib.ptmi_istft_forward(spec.data_ptr(), B, T, rf.data_ptr(), tb['syn'].data_ptr(), tb['twiddle'].data_ptr(), st._geom,
                                      0, 1.0, st._geom.pad_left, n, n, out.data_ptr(), _lib.stream(dev)), 'ptmi_istft_forward')
    G.check(G.blocks_of(out.cpu().numpy(), shift), G.blocks_of(wi, shift), G.blocks_of(ri, shift), 'inverse 512/128 ragged row_frames')


# ------------------------------------------------------------------------------------------------ 5. PIT features
def _cos_figure(cos, cos_want, Y_abs, X_abs):
    """``|cos - cos_want| min(|Y|, |X|) / max(||Y_t||, ||X_t||)``: what an error in the spectra can do to the cosine ([T, K, F])."""
    nrm = np.maximum(np.linalg.norm(Y_abs, axis=-1)[:, None], np.linalg.norm(X_abs, axis=-1))[..., None]
    w = np.minimum(Y_abs[:, None, :], X_abs) / np.where(nrm == 0, 1., nrm)
    return float((np.abs(cos.astype(np.float64) - cos_want) * w).max(initial=0.))


@pytest.mark.parametrize('K', [1, 3])
@pytest.mark.parametrize('size', [64, 512, 2048, 100])
def test_pit_features_ragged_with_nan_behind_the_rows(size, K):
    shift = size // 4
    N = 5 * size + 17
    lens = [N, N - 1, size + 1]
    rng = np.random.RandomState(size + K)
    s = rng.standard_normal((3, K, N)).astype(np.float32)
    y = (s.sum(1) + 0.5 * rng.standard_normal((3, N))).astype(np.float32)
    _check_features(y, s, lens, size, shift, f'features {size}/{shift} K={K}')


def _check_features(y, s, lens, size, shift, what):
    """``pit_features`` of the mixtures ``y [B, W]`` and sources ``s [B, K, W]`` with ``lens`` live samples per row, NaN behind them."""
    from padertorch_amd.ops import pit_features
    (B, K, W) = s.shape
    sf, yf = s.copy(), y.copy()
    for b, n in enumerate(lens):
        sf[b, :, n:] = np.nan
        yf[b, n:] = np.nan
    kw = _kw()
    f = pit_features(_dev(yf), _dev(sf), num_samples=lens, stft=_stft(size, shift, kw))
    Yg, Xg, Cg = (f[k].padded.cpu().numpy() for k in ('Y_abs', 'X_abs', 'cos_phase_difference'))
    T = stft_np.num_frames(max(lens), size, shift, 'full', True)
    F = size // 2 + 1
    assert W >= max(lens) and Yg.shape == (B, T, F) and Xg.shape == Cg.shape == (B, T, K, F)
    Yw, Y32 = np.zeros(Yg.shape), np.zeros(Yg.shape, np.float32)
    Xw, X32 = np.zeros(Xg.shape), np.zeros(Xg.shape, np.float32)
    q = q32 = 0.
    for b, n in enumerate(lens):
        r = features_np.pre_batch_transform(s[b, :, :n], y[b, :n], size, shift)
        Tb = r['num_frames']
        assert f['num_frames'][b] == Tb
        Yc = G.stft32(y[b, :n], size, shift, **kw)                               # [Tb, F] complex64
        Xc = np.transpose(G.stft32(s[b, :, :n], size, shift, **kw), (1, 0, 2))   # [Tb, K, F]
        Yw[b, :Tb], Xw[b, :Tb] = r['Y_abs'], r['X_abs']
        Y32[b, :Tb], X32[b, :Tb] = np.abs(Yc), np.abs(Xc)
        assert Y32.dtype == np.float32
        cos32 = np.cos(np.angle(Yc)[:, None, :] - np.angle(Xc))
        assert cos32.dtype == np.float32
        assert np.isfinite(Cg[b]).all() and (Cg[b, Tb:] == 0).all()
        q = max(q, _cos_figure(Cg[b, :Tb], r['cos_phase_difference'], r['Y_abs'], r['X_abs']))
        q32 = max(q32, _cos_figure(cos32, r['cos_phase_difference'], r['Y_abs'], r['X_abs']))
    G.check(Yg, Yw, Y32, f'{what} Y_abs')
    G.check(Xg, Xw, X32, f'{what} X_abs')
    print(f'gate {what} cos: max q {q:.3e}  max q32 {q32:.3e}  ratio {q / q32:.2f} (margin {G.MARGIN})')
    assert q <= G.MARGIN * q32, (q, q32)


# ------------------------------------------------------------------------------------------------ 6. MelTransform / mel_apply_kernel
def _spectrogram(rng, rows, F):
    """Non-negative float32, six decades of dynamic range across the bins."""
    decades = 10. ** (-6. * rng.permutation(F) / max(F - 1, 1))
    return (rng.random_sample((rows, F)) * decades).astype(np.float32)


def _mel_bounds(E_want, cnt, log, eps, lin_bound=None):
    """The derived bound of the (log-)mel outputs ``[..., M]``: ``lin_bound`` defaults to the non-negative dot product's
    ``(8 cnt[m] + 2) 2^-24 E_want``; in the log domain that over ``E_want + eps`` plus one rounding of ``acc + eps`` and the device
    ``logf``: ``4 spacing_fp32(|want|) + 2^-23``."""
    if lin_bound is None:
        lin_bound = (8. * cnt + 2.) * 2. ** -24 * E_want
    if not log:
        return lin_bound
    want = np.log(E_want + eps)
    return lin_bound / (E_want + eps) + 4. * np.spacing(np.abs(want).astype(np.float32)).astype(np.float64) + 2. ** -23


def _log_eps(eps):
    """``log(eps)`` as float32 arithmetic computes it, on the host and on the device (torch's own elementwise kernel, not the code
    under test).  The device ``logf`` is not correctly rounded - ``logf(1e-12f)`` is -27.631023 where the host's float32 log gives
    -27.631021, one spacing apart - so the host's value alone cannot serve as the exact one, and the device's alone would tie the
    tests to torch and the compiler sharing one ``logf``: both are float32 evaluations of ``log(eps)``, either is right."""
    host = np.log(np.float32(eps))
    dev = torch.log(torch.full((), eps, dtype=torch.float32, device=DEV)).cpu().numpy()[()]
    assert host.dtype == dev.dtype == np.float32
    for v in (host, dev):
        assert abs(float(v) - np.log(eps)) <= 4 * np.spacing(np.float32(abs(np.log(eps)))) + 2. ** -23
    return host, dev


def _all_log_eps(values, eps):
    """Outputs without energy (empty filters, frames past a row's end): ONE value bit for bit - nothing leaks into them - and that
    value a float32 ``log(eps)`` (:func:`_log_eps`)."""
    values = np.asarray(values)
    if values.size == 0:
        return True
    first = values.reshape(-1)[0]
    return bool((values == first).all()) and any(float(first) == float(v) for v in _log_eps(eps))


def _check_mel(mt, spec, what):
    fb = mt.fbanks.detach().cpu().numpy()
    assert fb.dtype == np.float32
    E_want = spec.astype(np.float64) @ fb.astype(np.float64)
    cnt = mt._bands.host['cnt'].astype(np.float64)
    got = mt(_dev(spec)).cpu().numpy().astype(np.float64)
    assert got.shape == E_want.shape and np.isfinite(got).all()
    want = np.log(E_want + mt.eps) if mt.log else E_want
    excess = np.abs(got - want) / _mel_bounds(E_want, cnt, mt.log, mt.eps).clip(1e-300)
    excess = np.where(np.abs(got - want) == 0, 0., excess)
    print(f'mel {what}: worst |error| / bound {excess.max():.3f}')
    assert excess.max() <= 1., (what, float(excess.max()))
    empty = np.flatnonzero(fb.sum(0) == 0)
    if len(empty):
        e = got[:, empty]
        assert _all_log_eps(e, mt.eps) if mt.log else (e == 0.).all(), what
    return len(empty)


@pytest.mark.parametrize('stft_size', [64, 128, 400, 512, 2048])          # F = 33, 65, 201, 257, 1025
def test_mel_transform_bound_per_filter(stft_size):
    from padertorch_amd.contrib.je.modules.features import MelTransform
    F = stft_size // 2 + 1
    rng = np.random.RandomState(F)
    specs = {rows: _spectrogram(rng, rows, F) for rows in [1, 7, 8, 9] + ([16387] if F == 33 else [])}
    for M in (1, 23, 80, 128):
        for log, eps in ((True, 1e-12), (True, 1e-3), (False, 1e-12)):
            mt = MelTransform(16000, stft_size, M, log=log, eps=eps).to(DEV)
            for rows, spec in specs.items():
                _check_mel(mt, spec, f'F={F} M={M} rows={rows} log={log} eps={eps}')


def test_mel_transform_empty_filters_give_log_eps_exactly():
    from padertorch_amd.contrib.je.modules.features import MelTransform
    spec = _spectrogram(np.random.RandomState(5), 9, 33)
    for log, eps in ((True, 1e-12), (True, 1e-3), (False, 1e-12)):
        mt = MelTransform(16000, 64, 80, log=log, eps=eps).to(DEV)
        assert _check_mel(mt, spec, f'80 filters on stft 64 log={log} eps={eps}') > 0


@pytest.mark.parametrize('stft_size', [64, 128, 400, 512])
def test_mel_transform_dense_user_filterbank(stft_size):
    """Every filter spans all bins: the last 8-bin group of each reaches past ``F`` (``F`` = 33, 65, 201, 257 is 1 mod 8)."""
    from padertorch_amd.contrib.je.modules.features import MelTransform
    F = stft_size // 2 + 1
    rng = np.random.RandomState(stft_size)
    dense = rng.random_sample((23, F)) + 0.05
    for log in (True, False):
        mt = MelTransform(16000, stft_size, 23, log=log, fbanks=dense).to(DEV)
        assert (mt._bands.host['cnt'] == (F + 7) // 8).all() and (mt._bands.host['cnt'] * 8 > F).all()
        for rows in (7, 9):
            _check_mel(mt, _spectrogram(rng, rows, F), f'dense F={F} rows={rows} log={log}')


# ------------------------------------------------------------------------------------------------ 7. fused stft_logmel
def _check_logmel(x, lens, size, shift, kw, mel_kw, what, xd=None, spectra=None):
    """All of ``power`` in (1, 2) x ``log`` on / off of one (signal, STFT, filterbank) case; ``lens``: ragged lengths or None;
    ``xd``: the device tensor to feed (default: a fresh copy of the signal); ``spectra``: the case's (fp64 oracle, fp32 restatement)
    where a test has them already."""
    from padertorch_amd.contrib.je.modules.features import MelTransform, stft_logmel
    st = _stft(size, shift, kw)
    B, N = x.shape
    T = stft_np.num_frames(N, kw['window_length'] or size, shift, kw['fading'], kw['pad'])
    F = size // 2 + 1
    if lens is None:
        X64, X32 = stft_np.stft(x, size, shift, **kw), G.stft32(x, size, shift, **kw)
        xf, live = x, np.ones((B, T), bool)
    else:
        if spectra is not None:
            X64, X32 = spectra
        else:
            X64 = _ragged_rows(lambda r: stft_np.stft(r, size, shift, **kw), x, lens, T, (F,), np.complex128)
            X32 = _ragged_rows(lambda r: G.stft32(r, size, shift, **kw), x, lens, T, (F,), np.complex64)
        xf = x.copy()
        live = np.zeros((B, T), bool)
        for b, n in enumerate(lens):
            xf[b, n:] = 1e30 if b % 2 else np.nan
            live[b, :stft_np.num_frames(n, kw['window_length'] or size, shift, kw['fading'], kw['pad'])] = True
    assert X64.shape == (B, T, F)
    xd = _dev(xf) if xd is None else xd
    mels = {log: MelTransform(16000, size, log=log, **mel_kw).to(DEV) for log in (True, False)}
    fb = mels[True].fbanks.detach().cpu().numpy()
    eps = mels[True].eps
    for power in (1, 2):
        P64 = np.abs(X64) ** power
        A32 = np.abs(X32)
        P32 = A32 * A32 if power == 2 else A32
        assert P32.dtype == np.float32
        E_want, E32 = P64 @ fb.astype(np.float64), P32 @ fb
        assert E32.dtype == np.float32
        maxP = P64.max(-1)
        lin = stft_logmel(xd, st, mels[False], num_samples=lens, power=power).cpu().numpy()
        assert lin.shape == E_want.shape
        assert (lin[~live] == 0).all()
        G.check(lin, E_want, E32, f'logmel {what} power={power} linear', norm=maxP)
        r32 = G.gate_figures(E32, E_want, E32, norm=maxP)[1]
        got = stft_logmel(xd, st, mels[True], num_samples=lens, power=power).cpu().numpy()
        assert np.isfinite(got).all()
        assert _all_log_eps(got[~live], eps)
        bound = _mel_bounds(E_want, None, True, eps, lin_bound=(G.MARGIN * r32 * maxP)[..., None])
        excess = np.abs(got.astype(np.float64) - np.log(E_want + eps)) / bound
        print(f'logmel {what} power={power} log: worst |error| / bound {excess.max():.3f}')
        assert excess.max() <= 1., (what, power, float(excess.max()))


@pytest.mark.parametrize('size', PLANS)
def test_logmel_every_plan(size):
    shift = size // 4
    x, kw, _, _ = _case(size, shift)
    _check_logmel(x, None, size, shift, kw, dict(number_of_filters=min(80, size // 4)), f'{size}/{shift}')


def test_logmel_128_filters_at_512():
    x, kw, _, _ = _case(512, 128)
    _check_logmel(x, None, 512, 128, kw, dict(number_of_filters=128), '512/128 M=128')


@pytest.mark.parametrize('size', [64, 512])
@pytest.mark.parametrize('opt', list(_options(64)))
def test_logmel_load_path_options(size, opt):
    shift = _options(size)[opt][0]
    x, kw, _, _ = _case(size, shift, opt)
    _check_logmel(x, None, size, shift, kw, dict(number_of_filters=min(80, size // 4)), f'{size}/{shift} {opt}')


@pytest.mark.parametrize('size', [64, 512])
def test_logmel_from_a_pointer_that_is_not_8_byte_aligned(size):
    """``stft_logmel`` hands the kernel the pointer of its own ``reshape(-1, N).contiguous()``: a contiguous view keeps its offset."""
    shift = size // 4
    x, kw, _, _ = _case(size, shift)
    N = x.shape[1]
    v = _misaligned_row(x[1]).unsqueeze(0)
    assert v.reshape(-1, N + 1).contiguous().data_ptr() == v.data_ptr()
    xr = np.zeros((1, N + 1), np.float32)
    xr[0, :N] = x[1]
    _check_logmel(xr, [N], size, shift, kw, dict(number_of_filters=min(80, size // 4)), f'{size}/{shift} misaligned', xd=v)


@pytest.mark.parametrize('size', [64, 256, 2048])
@pytest.mark.parametrize('width', [0, 1])
def test_logmel_ragged_rows_with_garbage_behind(size, width):
    """``width`` = 1: an even row stride, i.e. the 8-byte load paths (see ``test_forward_ragged_rows_with_live_padding``)."""
    shift = size // 4
    N = 5 * size + 17
    lens = _ragged_lengths(size, shift, N)
    x = np.random.RandomState(size + 2).standard_normal((len(lens), N + width)).astype(np.float32)
    _check_logmel(x, lens, size, shift, _kw(), dict(number_of_filters=min(80, size // 4)), f'{size}/{shift} ragged width N+{width}')


@pytest.mark.parametrize('size', [64, 512])
def test_logmel_dense_user_filterbank(size):
    """Every filter's last 8-bin group reaches past bin ``F`` (the zeroed pad behind the spectrum in LDS)."""
    shift = size // 4
    x, kw, _, _ = _case(size, shift)
    dense = np.random.RandomState(size).random_sample((16, size // 2 + 1)) + 0.05
    _check_logmel(x, None, size, shift, kw, dict(number_of_filters=16, fbanks=dense), f'{size}/{shift} dense')


# ------------------------------------------------------------------------------------------------ 8. a wavefront that takes several items
# The cases above give every wavefront of the forward kernels at most one work item (FPW frames of one row).  A CU holds at most 8
# wavefronts per SIMD, 256 CUs at most 8192 whatever a kernel's occupancy, so the 20 484 items of these shapes give every wavefront
# two or three: the prefetch carried from item to item, the hand-over between interior and edge items and the run past the last
# item.  Size 64 / shift 16 (8 frames per item); 4 rows of N = 655 377 samples (odd) in N + 1 columns (an even stride: the 8-byte
# loads and the separately fetched last sample), NaN behind every row's end; the lengths make interior, edge and all-past-the-end
# items alternate within a wavefront's stride.
MULTI = dict(size=64, shift=16, N=655377)


def _multi_lengths():
    N = MULTI['N']
    return [N, N - 1, N // 2 + 3, 5]


@pytest.fixture(scope='module')
def multi_case():
    """(x float32 [4, N + 1], lengths, frames of the buffer, want complex128, ref32 complex64): computed once for this module's
    cases, read-only, released with the module (about 130 MB)."""
    size, shift, N = MULTI['size'], MULTI['shift'], MULTI['N']
    lens = _multi_lengths()
    kw = _kw()
    x = np.random.RandomState(N).standard_normal((len(lens), N + 1)).astype(np.float32)
    T = stft_np.num_frames(N + 1, size, shift, 'full', True)
    F = size // 2 + 1
    want = _ragged_rows(lambda r: stft_np.stft(r, size, shift, **kw), x, lens, T, (F,), np.complex128)
    ref32 = _ragged_rows(lambda r: G.stft32(r, size, shift, **kw), x, lens, T, (F,), np.complex64)
    assert len(lens) * ((T + 7) // 8) > 2 * 8192
    for a in (x, want, ref32):
        a.setflags(write=False)
    return x, lens, T, want, ref32


def _nan_behind(x, lens):
    xf = x.copy()
    for b, n in enumerate(lens):
        xf[b, n:] = np.nan
    return xf


def test_multi_item_forward(multi_case):
    size, shift = MULTI['size'], MULTI['shift']
    x, lens, T, want, ref32 = multi_case
    v = _dev(_nan_behind(x, lens))
    assert v.data_ptr() % 8 == 0 and v.stride(0) % 2 == 0 and lens[0] % 2 == 1
    X = _stft(size, shift, _kw())(v, num_samples=torch.tensor(lens, dtype=torch.int32, device=DEV)).cpu().numpy()
    assert X.shape == want.shape and not np.isnan(X).any()
    for b, n in enumerate(lens):
        assert (X[b, stft_np.num_frames(n, size, shift, 'full', True):] == 0).all(), b
    G.check(X, want, ref32, f'forward {size}/{shift} multi-item')


def test_multi_item_pit_features(multi_case):
    """K = 1: the same rows as mixtures, one array of sources.  The items go frame-group major, so the same lengths interleave
    otherwise than in the forward kernel."""
    size, shift = MULTI['size'], MULTI['shift']
    x, lens, _, _, _ = multi_case
    s = np.random.RandomState(MULTI['N'] + 1).standard_normal((len(lens), 1, x.shape[1])).astype(np.float32)
    _check_features(x, s, lens, size, shift, f'features {size}/{shift} K=1 multi-item')


def test_multi_item_logmel(multi_case):
    size, shift = MULTI['size'], MULTI['shift']
    x, lens, _, want, ref32 = multi_case
    _check_logmel(x, lens, size, shift, _kw(), dict(number_of_filters=min(80, size // 4)), f'{size}/{shift} multi-item',
                  spectra=(want, ref32))


def test_multi_item_griffin_lim_step():
    """One fused iteration (``gl_stft_update_kernel``) against the composed path, as ``tests/test_gpu_griffin_lim.py``
    (``test_fused_against_composed``) compares them: 2e-4 max(a), the floor of its gate (one step is the forward and the inverse
    STFT gate taken together), and the RMSE (the fp64 sum in item order over every wavefront's items) to 1e-4.  Both paths take
    their STFT through the same ``wave_pipeline``, so an error in the carried prefetch or the interior / edge hand-over would cancel
    here (``x`` comes out bit-identical): this case gates the Griffin-Lim epilogue and its item-order sum over several items only;
    the pipeline itself is held against the fp64 oracle by ``test_multi_item_forward``."""
    from padertorch_amd.contrib.mk.synthesis import fast_griffin_lim
    from padertorch_amd.ops import griffin_lim as gl
    size, shift, B, T = MULTI['size'], MULTI['shift'], 4, 40962
    F = size // 2 + 1
    rng = np.random.RandomState(T)
    a = _dev(np.abs(rng.standard_normal((B, T, F))).astype(np.float32))
    x0 = _dev((rng.standard_normal((B, T, F)) + 1j * rng.standard_normal((B, T, F))).astype(np.complex64))
    st = _stft(size, shift, _kw())
    out = {}
    before = gl.PATH
    try:
        for path in ('fused', 'composed'):
            gl.PATH = path
            out[path] = fast_griffin_lim(a, st, alpha=0.99, iterations=1, atol=0., x=x0, return_info=True)[1]
    finally:
        gl.PATH = before
    f, c = out['fused'], out['composed']
    assert int(f.num_iterations) == int(c.num_iterations) == 1 and bool(torch.isfinite(f.x.abs()).all())
    dev = float((f.x - c.x).abs().max()) / float(a.max())
    rel = float(((f.rmse - c.rmse).abs() / c.rmse).max())
    print(f'gate griffin-lim {size}/{shift} multi-item: fused vs composed {dev:.3g} (gate 2e-4), ratio {dev / 2e-4:.2f}; rmse {rel:.3g}')
    assert dev <= 2e-4 and rel <= 1e-4


# ------------------------------------------------------------------------------------------------ 9. what cannot fit says so
def test_logmel_request_beyond_lds_names_lds():
    from padertorch_amd.contrib.je.modules.features import MelTransform, stft_logmel
    x, kw, _, _ = _case(1024, 256)
    dense = np.random.RandomState(0).random_sample((80, 513)) + 0.05
    mt = MelTransform(16000, 1024, 80, fbanks=dense).to(DEV)
    with pytest.raises(NotImplementedError, match='LDS'):
        stft_logmel(_dev(x), _stft(1024, 256, kw), mt)
