"""The STFT coders of the reference's TasNet (``StftEncoder`` / ``IstftDecoder``, ``tasnet/tas_coders.py:138-240``) as FIXED-BASIS coders
on the kernels of ``csrc/tas_coders.hip``.

At TasNet geometry (windows of 16-20 samples, a hop of half a window) an STFT is no FFT problem: the reference itself computes it as
``conv1d`` with a constant ``[N, 1, L]`` kernel (``get_stft_kernel``, ``_stft.py:11-23``) and the inverse as two ``conv_transpose1d``
(``get_istft_kernel``, ``:26-43``).  That is the operator pair of the learned coders (``ops/tas.py``) with a basis that has no gradient:

    stft_bases(window_length, feature_size, stride, window)   the two bases ``[N, L]``, fp64 on the host, rounded once to fp32
    stft_encode(x, analysis, stride)                          conv1d(zero-padded x)        ``[B, T] -> [B, N, E]``   (``tas_analysis``, no ReLU)
    istft_decode(w, synthesis, stride)                        conv_transpose1d(w)[:, 0]    ``[B, N, E] -> [B, T']``  (``tas_synthesis``)
    istft_masked_decode(mask, encoded, synthesis, stride)     istft_decode(mask[k] * encoded) for every k, the product never in memory

``N = feature_size`` (even), the transform size is ``N - 2`` with ``F = N / 2`` bins; a feature column holds the ``F`` real parts on top
of the ``F`` imaginary parts (``complex_representation='concat'``, transposed).  Each operator is differentiable in its signal inputs; the
adjoint of the analysis is the synthesis kernel with the same basis and the other way round, so no backward ever launches ``tas_wgrad``.
fp32 on the GPU only, with the checks and error texts of ``ops/tas.py``.

The path is designed and measured for TasNet-sized windows (``profiles/stft_tasnet.txt``).  Every geometry the coder kernels accept is
correct - they have generic paths above 32 taps and above the LDS-staged basis size - but a dense basis at, say, size 512 / shift 128
does ``N L`` multiply-adds per sample where an FFT does ``N log N`` per frame and is NOT tuned; ``ops.STFT`` is the path for that.
"""
import numpy as np
import torch
from torch.autograd.function import once_differentiable

from . import library  # noqa: F401  (registers torch.ops.ptmi.*)
from ._stft import _biorthogonal_window
from .. import _lib

__all__ = ['stft_bases', 'stft_frames', 'stft_encoded_lengths', 'stft_encode', 'istft_decode', 'istft_masked_decode']


def stft_bases(window_length, feature_size, stride, window):
    """``(analysis [N, L], synthesis [N, L])`` as float32 CPU tensors; ``window`` is the fp64 analysis window of ``ops.STFT``
    (``STFT.window``, ``window_length`` long).

    ``analysis``: rows ``0 .. F-1`` the real and rows ``F .. N-1`` the imaginary parts of ``window[l] exp(-2 pi i f l / size)``
    (``get_stft_kernel``, squeezed).  ``synthesis``: the reference applies two ``[size, 1, L]`` kernels ``k_re`` / ``k_im`` (biorthogonal
    window and ``1 / size`` inside) to the Hermitian extension of the ``F`` bins (``_stft.py:243-247``: bin ``size - f`` is the conjugate of
    bin ``f``); folded into the ``F`` bins that is ``b_re[f] = k_re[f] + k_re[size - f]`` and ``b_im[f] = k_im[f] - k_im[size - f]`` for
    ``0 < f < F - 1``, and the kernels' own rows for ``f = 0`` and ``f = F - 1``, which have no mirror."""
    L, N = int(window_length), int(feature_size)
    window = np.asarray(window, dtype=np.float64)
    if N < 4 or N % 2 or window.shape != (L,) or L > N - 2 or stride < 1:
        raise ValueError(f'stft_bases: an even feature_size >= 4, a window of window_length <= feature_size - 2 samples and a stride >= 1, '
                         f'got window_length {L}, feature_size {N}, stride {stride}, window {window.shape}')
    size, F = N - 2, N // 2
    tap = np.arange(L)[None, :]
    ang = -1 * np.arange(F)[:, None] * 2 * np.pi / size * tap
    analysis = np.concatenate([np.cos(ang) * window, np.sin(ang) * window], axis=0)
    syn = _biorthogonal_window(window, stride) / size
    ang = np.arange(size)[:, None] * 2 * np.pi / size * tap
    k_re, k_im = np.cos(ang) * syn, np.sin(-ang) * syn
    b_re, b_im = k_re[:F].copy(), k_im[:F].copy()
    b_re[1:F - 1] += k_re[:F - 1:-1]                                       # rows size - 1 ... F of the mirror half
    b_im[1:F - 1] -= k_im[:F - 1:-1]
    synthesis = np.concatenate([b_re, b_im], axis=0)
    return torch.from_numpy(analysis.astype(np.float32)), torch.from_numpy(synthesis.astype(np.float32))


def stft_frames(samples, window_length, stride):
    """Frames the encoder returns for a batch that is ``samples`` long: ``ceil((samples - L) / stride) + 1``, and one frame for anything
    shorter than a window (the reference pads that up to one window, ``_stft.py:148-154``)."""
    if samples < 1:
        raise RuntimeError(f'stft_encode: {samples} samples')
    return max(-((window_length - samples) // stride) + 1, 1)


def stft_encoded_lengths(sequence_lengths, window_length, stride):
    """``ceil((n - L) / stride) + 1`` for every entry: the reference's ``samples_to_frames`` without fading (zero or negative below
    ``L - stride`` samples, as there).  A list or a CPU tensor gives a CPU int64 tensor; a CUDA tensor is computed on its device, in its
    integer dtype, with no synchronisation."""
    if sequence_lengths is None:
        return None
    n = sequence_lengths if torch.is_tensor(sequence_lengths) else torch.tensor([int(v) for v in sequence_lengths], dtype=torch.int64)
    if not n.is_cuda:
        n = n.to(torch.int64)
    elif n.is_floating_point():
        raise NotImplementedError(f'stft_encoded_lengths: integer lengths, got {n.dtype}')
    return 1 - torch.div(window_length - n, stride, rounding_mode='floor')


def _check(name, *tensors):
    """The checks and error texts of ``ops/tas.py``; the dtype first, so that it is refused with or without a GPU."""
    for t in tensors:
        if t.dtype != torch.float32:
            raise NotImplementedError(f'{name}: float32 only, got {t.dtype}')
    _lib.require_gpu(*tensors)


class _StftEncodeFn(torch.autograd.Function):
    """Kernels: ``tas_analysis`` (linear) forward, ``tas_synthesis`` (un-gated, the same basis) backward.  No activation is saved: the
    basis is a constant buffer of the coder, and the map is linear."""

    @staticmethod
    def forward(ctx, x, basis, stride, frames):
        ctx.basis, ctx.stride, ctx.samples = basis, stride, x.shape[1]
        return torch.ops.ptmi.tas_analysis(x.contiguous(), basis, None, stride, frames, False)

    @staticmethod
    @once_differentiable
    def backward(ctx, gw):
        return torch.ops.ptmi.tas_synthesis(gw.contiguous(), None, None, ctx.basis, None, ctx.stride, ctx.samples), None, None, None


class _IstftDecodeFn(torch.autograd.Function):
    """Kernels: ``tas_synthesis`` forward, ``tas_analysis`` (linear, the same basis) backward."""

    @staticmethod
    def forward(ctx, w, basis, stride):
        ctx.basis, ctx.stride, ctx.frames = basis, stride, w.shape[2]
        samples = (w.shape[2] - 1) * stride + basis.shape[-1]
        return torch.ops.ptmi.tas_synthesis(w.contiguous(), None, None, basis, None, stride, samples)

    @staticmethod
    @once_differentiable
    def backward(ctx, gy):
        return torch.ops.ptmi.tas_analysis(gy.contiguous(), ctx.basis, None, ctx.stride, ctx.frames, False), None, None


class _IstftMaskedDecodeFn(torch.autograd.Function):
    """Kernels: ``tas_synthesis`` (masked) forward, ``tas_masked_decode_backward`` backward."""

    @staticmethod
    def forward(ctx, mask, encoded, basis, stride):
        mask, encoded = mask.contiguous(), encoded.contiguous()
        samples = (encoded.shape[2] - 1) * stride + basis.shape[-1]
        ctx.save_for_backward(mask, encoded)
        ctx.basis, ctx.stride = basis, stride
        return torch.ops.ptmi.tas_synthesis(encoded, mask, None, basis, None, stride, samples)

    @staticmethod
    @once_differentiable
    def backward(ctx, gy):
        mask, encoded = ctx.saved_tensors
        dm, de = torch.ops.ptmi.tas_masked_decode_backward(gy.contiguous(), mask, encoded, ctx.basis, ctx.stride)
        return (dm if ctx.needs_input_grad[0] else None), (de if ctx.needs_input_grad[1] else None), None, None


def _basis(name, basis, stride):
    """The basis as the kernels read it: ``[N, L]``, contiguous, without a gradient."""
    if basis.dim() == 3 and basis.shape[1] == 1:
        basis = basis[:, 0]
    if basis.dim() != 2 or basis.shape[0] % 2 or stride < 1:
        raise ValueError(f'{name}: basis [N, L] with an even N and a stride >= 1, got {tuple(basis.shape)}, stride {stride}')
    if basis.requires_grad:
        raise ValueError(f'{name}: the basis is fixed and has no gradient; a learned basis is ops.tas_encode / tas_decode')
    return basis.contiguous()


def stft_encode(x, analysis, stride):
    """``conv1d(pad(x)[:, None], analysis[:, None], stride)`` for ``x [B, T]``: ``[B, N, E]``, contiguous, ``E = stft_frames(T, L, stride)``.
    The samples behind ``T`` that the last frame covers read as zeros in the kernel; nothing is padded in memory."""
    _check('stft_encode', x, analysis)
    analysis = _basis('stft_encode', analysis, stride)
    if x.dim() != 2:
        raise ValueError(f'stft_encode: x [B, T], got {tuple(x.shape)}')
    return _StftEncodeFn.apply(x, analysis, int(stride), stft_frames(x.shape[1], analysis.shape[1], int(stride)))


def istft_decode(w, synthesis, stride):
    """``conv_transpose1d(w, synthesis[:, None], stride)[:, 0]`` for ``w [B, N, E]``: ``[B, (E - 1) stride + L]``."""
    _check('istft_decode', w, synthesis)
    synthesis = _basis('istft_decode', synthesis, stride)
    if w.dim() != 3 or w.shape[1] != synthesis.shape[0]:
        raise ValueError(f'istft_decode: w [B, {synthesis.shape[0]}, frames], got {tuple(w.shape)}')
    return _IstftDecodeFn.apply(w, synthesis, int(stride))


def istft_masked_decode(mask, encoded, synthesis, stride):
    """``istft_decode(mask[k] * encoded)`` for every ``k``: ``mask [K, B, N, E]``, ``encoded [B, N, E]`` -> ``[K, B, (E - 1) stride + L]``.
    The product never exists in memory, forward or backward."""
    _check('istft_masked_decode', mask, encoded, synthesis)
    synthesis = _basis('istft_masked_decode', synthesis, stride)
    if encoded.dim() != 3 or mask.dim() != 4 or tuple(mask.shape[1:]) != tuple(encoded.shape) or encoded.shape[1] != synthesis.shape[0]:
        raise ValueError(f'istft_masked_decode: mask [K, B, N, frames] and encoded [B, N, frames] with N = {synthesis.shape[0]}, got '
                         f'{tuple(mask.shape)}, {tuple(encoded.shape)}')
    return _IstftMaskedDecodeFn.apply(mask, encoded, synthesis, int(stride))
