"""Per-frame accuracy gate for the spectral kernels.  ORACLE - test infrastructure only (numpy / torch CPU).

A whole-tensor gate ``atol = c * max|ref|`` says nothing about frames that are small against the tensor's maximum - the fading
frames at both ends, the last frame of an odd-length row (which may hold ONE sample under a window tap of 1e-17) - and these are
the frames with load paths of their own.  The gate here is per row and frame:

    r[b, t] = max_k |got[b, t, k] - want[b, t, k]| / || want[b, t, :] ||_2

with ``want`` from the fp64 oracle (:mod:`oracle.stft_np`); a frame that is exactly zero in the oracle must be exactly zero in
``got``.  What ``r`` may be is not a constant but what fp32 arithmetic itself costs on the same case: ``r32``, the same figure of
an fp32 RESTATEMENT of the transform (:func:`stft32`, :func:`istft32`: framing as ``stft_np``, fp32 window multiply, ``torch.fft``
on float32 on the CPU, fp32 overlap-add) that never touches the code under test.  Gate: ``max r <= MARGIN * max r32``, maxima
pooled over the frames of the case.

``MARGIN = 8``: the kernels' packed real FFT has one stage more than the restatement (the hermitian split), its twiddles are fp32
table entries rounded at 6e-8 each, and its R1 x R2 factorisation differs from pocketfft's; all of that grows like
``eps * log2(size)``, as the restatement does.  It is never derived from a kernel's own output.
"""
import numpy as np
import torch

from . import stft_np

MARGIN = 8


# --------------------------------------------------------------------------- framing (as stft_np.stft)
def frames_of(x, size, shift, *, window='blackman', window_length=None, fading='full', pad=True, symmetric_window=False):
    """The unwindowed frames ``[..., n, L]`` (float64) and the window ``[L]`` (float64) of ``stft_np.stft(x, ...)``."""
    x = np.asarray(x, dtype=np.float64)
    L = size if window_length is None else window_length
    w = stft_np.get_window(window, symmetric_window, L)
    left, T = stft_np.padded_length(x.shape[-1], L, shift, fading, pad)
    xp = np.zeros(x.shape[:-1] + (max(T, left + x.shape[-1]),))
    xp[..., left:left + x.shape[-1]] = x
    n = (T - L) // shift + 1
    idx = np.arange(L)[None, :] + shift * np.arange(n)[:, None]
    return xp[..., idx], w


def stft32(x, size, shift, **kw):
    """fp32 restatement of ``stft_np.stft``: float32(frames) * float32(window) in fp32, ``torch.fft.rfft`` on float32 -> complex64."""
    fr, w = frames_of(x, size, shift, **kw)
    f32 = torch.from_numpy(fr.astype(np.float32)) * torch.from_numpy(w.astype(np.float32))
    assert f32.dtype == torch.float32
    X = torch.fft.rfft(f32, n=size, dim=-1)
    assert X.dtype == torch.complex64, X.dtype
    return X.numpy()


def istft32(X, size, shift, *, window='blackman', window_length=None, fading='full', symmetric_window=False):
    """fp32 restatement of ``stft_np.istft``: ``torch.fft.irfft`` on complex64, fp32 synthesis-window multiply, fp32 overlap-add."""
    from math import ceil
    L = size if window_length is None else window_length
    ws = stft_np.biorthogonal_window(stft_np.get_window(window, symmetric_window, L), shift)
    Xc = torch.from_numpy(np.ascontiguousarray(np.asarray(X).astype(np.complex64)))
    fr = torch.fft.irfft(Xc, n=size, dim=-1)
    assert fr.dtype == torch.float32, fr.dtype
    fr = fr[..., :L] * torch.from_numpy(ws.astype(np.float32))
    n = Xc.shape[-2]
    out = torch.zeros(Xc.shape[:-2] + ((n - 1) * shift + L,), dtype=torch.float32)
    for t in range(n):
        out[..., t * shift:t * shift + L] += fr[..., t, :]
    if fading not in (None, False):
        pw = L - shift
        if fading == 'half':
            pw = pw / 2
        out = out[..., int(pw):out.shape[-1] - ceil(pw)]
    return out.numpy()


# --------------------------------------------------------------------------- the gate
def frame_ratio(got, want, norm=None):
    """``r[..., t] = max_k |got - want| / ||want[..., t, :]||_2`` over the last axis (float64); ``norm[..., t]`` replaces the l2 norm
    where the issue at hand defines another yardstick per frame (the fused mel energies: the frame's largest spectral power).

    Raises ``AssertionError`` if ``got`` holds a non-finite value or is not exactly zero in a frame that is exactly zero in ``want``
    (frames past a ragged row's end, frames wholly in padding); such frames count 0."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (got.shape, want.shape)
    assert np.isfinite(got).all(), f'{int((~np.isfinite(got)).sum())} non-finite values'
    cplx = np.iscomplexobj(want) or np.iscomplexobj(got)
    got = got.astype(np.complex128 if cplx else np.float64)
    want = want.astype(np.complex128 if cplx else np.float64)
    nrm = np.sqrt((np.abs(want) ** 2).sum(-1)) if norm is None else np.broadcast_to(np.asarray(norm, np.float64), want.shape[:-1])
    err = np.abs(got - want).max(-1) if want.shape[-1] else np.zeros(want.shape[:-1])
    zero = nrm == 0
    assert not (np.abs(got).max(-1)[zero] != 0).any(), \
        f'{int((np.abs(got).max(-1)[zero] != 0).sum())} frames that are exactly zero in the oracle are not zero'
    return np.where(zero, 0., err / np.where(zero, 1., nrm))


def blocks_of(x, shift):
    """``[..., N]`` -> ``[..., ceil(N / shift), shift]`` (zero-filled tail): the inverse's "frames" are blocks of ``shift`` samples."""
    x = np.asarray(x)
    n = x.shape[-1]
    nb = -(-n // shift)
    out = np.zeros(x.shape[:-1] + (nb * shift,), x.dtype)
    out[..., :n] = x
    return out.reshape(x.shape[:-1] + (nb, shift))


def gate_figures(got, want, ref32, norm=None):
    """``(max r, max r32)`` of a case, maxima pooled over its rows and frames (``ref32``: the fp32 restatement's result)."""
    return float(frame_ratio(got, want, norm).max(initial=0.)), float(frame_ratio(ref32, want, norm).max(initial=0.))


def passes(got, want, ref32, margin=MARGIN, norm=None):
    """The gate as a predicate (a zero-frame / non-finite violation counts as a failure)."""
    try:
        r, r32 = gate_figures(got, want, ref32, norm)
    except AssertionError:
        return False
    return r <= margin * r32


def check(got, want, ref32, what, margin=MARGIN, norm=None):
    """Assert the gate; prints the measured ratio ``max r / max r32`` of the case and returns it."""
    r, r32 = gate_figures(got, want, ref32, norm)
    ratio = r / r32 if r32 > 0 else (0. if r == 0 else float('inf'))
    print(f'gate {what}: max r {r:.3e}  max r32 {r32:.3e}  ratio {ratio:.2f} (margin {margin})')
    assert r <= margin * r32, f'{what}: max r {r:.3e} > {margin} * max r32 {r32:.3e} (ratio {ratio:.2f})'
    return ratio


def old_gate_passes(got, want, c=2e-4):
    """The whole-tensor gate of tests/test_gpu_stft.py: ``atol = c * max|want|``."""
    return bool(np.abs(np.asarray(got) - np.asarray(want)).max() <= c * np.abs(want).max())
