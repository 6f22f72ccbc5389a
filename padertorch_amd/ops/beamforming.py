"""Mask-based MVDR beamforming on the HIP kernels of ``csrc/beamform.hip``: what a speech and a noise mask are estimated for
(``padertorch/contrib/examples/speech_enhancement/mask_estimator/evaluate.py:110-137``, ``contrib/jensheit/evaluation.py:14-45``).
The reference does this on the host with the third-party ``pb_bss`` / ``paderbox``; the functions here restate their documented
behaviour in the layout ``ops.STFT`` and the estimators produce, and nothing leaves the device.

    observation, mix  ``[B, C, T, F]`` complex64 (``[C, T, F]``: ``B = 1``), ``1 <= C <= 8`` channels
    mask              ``[B, C, T, F]`` float32, or ``[B, T, F]`` when already reduced over the channels
    frames            optional ``[B]`` int32 on the device: frames ``t >= frames[b]`` contribute nothing and come out as zero

    get_power_spectral_density_matrix(observation, mask=None, *, frames=None, channel_reduce='median', normalize=True)
        ``Phi[b,f,d,e] = sum_t m[b,t,f] Y[b,d,t,f] conj(Y[b,e,t,f]) / max(sum_t m[b,t,f], 1e-10)`` -> ``[B, F, C, C]`` complex128,
        exactly Hermitian.  ``m`` is the median of the mask over the channels (numpy's: for even ``C`` the mean of the two middle
        values); ``channel_reduce=None`` takes a ``[B, T, F]`` mask as it is; ``mask=None`` is the covariance over the valid frames;
        ``normalize=False`` does not divide.
    get_mvdr_vector_souden(target_psd_matrix, noise_psd_matrix, ref_channel=None, *, return_ref_channel=False)
        ``X = Phi_n^-1 Phi_s`` (solved with partial pivoting, not inverted), ``M = X / max(Re trace X, tiny)`` with ``tiny`` the
        smallest normal float64, ``w[b,f,:] = M[b,f,:,ref]`` -> ``[B, F, C]`` complex64.  ``ref_channel=None`` picks, per example,
        ``argmax_r Re(sum_f w_r^H Phi_s w_r) / max(Re(sum_f w_r^H Phi_n w_r), tiny)`` (a ratio of sums over the bins, first maximum)
        on the device; ``return_ref_channel`` also returns the choice as a ``[B]`` int32 tensor.  Nothing synchronises.
        A pivot that is exactly zero leaves the unknowns of its column zero, so a bin whose ``Phi_n`` is all zero (its noise mask is
        zero everywhere) gives ``w = 0`` and a zero output - as the least-squares fallback of the reference's solver does.  A
        rank-deficient but non-zero ``Phi_n`` (``frames[b] < C``) is NOT guarded, exactly as upstream: the result is whatever the
        elimination gives.
    apply_beamforming_vector(vector, mix, *, frames=None)
        ``Z[b,t,f] = sum_c conj(vector[b,f,c]) mix[b,c,t,f]`` -> ``[B, T, F]`` complex64
    mask_beamforming(observation, speech_mask, noise_mask, *, frames=None, ref_channel=None)
        the three together -> ``Z [B, T, F]``: both PSD matrices from ONE pass over the observation, three launches plus the
        reference-channel stage.

Inference only: an input that requires grad raises.  complex64 / float32 (PSD matrices complex128) on the GPU only: other dtypes
raise ``NotImplementedError``, CPU tensors the "no CPU fallback" error; more than 8 channels raise ``NotImplementedError``.
"""
import torch

from .. import _lib
from . import library  # noqa: F401  (registers torch.ops.ptmi.*)

__all__ = ['get_power_spectral_density_matrix', 'get_mvdr_vector_souden', 'apply_beamforming_vector', 'mask_beamforming',
           'MAX_CHANNELS']

#: the kernels keep a bin's C (C + 1) / 2 products per mask in registers
MAX_CHANNELS = 8


def _check(name, dtypes, *tensors):
    """``dtypes``: one per tensor (None entries of ``tensors`` are absent operands).  What an argument IS (dtype, shape, channels,
    requires grad) is refused before where it lives (``_lib.require_gpu``, called by the functions behind their shape checks)."""
    for t, dtype in zip(tensors, dtypes):      # (the dtype first: a float64 mask is refused for what it is, wherever it lives)
        if t is not None and t.dtype != dtype:
            raise NotImplementedError(f'{name}: {dtype} only, got {t.dtype}')
    for t in tensors:
        if t is not None and t.requires_grad:
            raise NotImplementedError(f'{name} is inference only (no backward), but an input requires grad')


def _channels(name, C):
    if C > MAX_CHANNELS:
        raise NotImplementedError(f'{name}: at most {MAX_CHANNELS} channels, got {C}')
    if C < 1:
        raise ValueError(f'{name}: no channels')


def _spectrum(name, x):
    """``[C, T, F]`` or ``[B, C, T, F]`` -> contiguous ``[B, C, T, F]`` and whether a batch axis was added."""
    if x.dim() not in (3, 4) or x.numel() == 0:
        raise ValueError(f'{name}: [B, C, T, F] or [C, T, F] spectra, got {tuple(x.shape)}')
    squeeze = x.dim() == 3
    x = x[None] if squeeze else x
    _channels(name, x.shape[1])
    return x.contiguous(), squeeze


def _mask(name, mask, shape, squeeze, reduce):
    """A mask for ``shape = (B, C, T, F)``: ``[B, C, T, F]`` (``reduce``) or ``[B, T, F]``, without the batch axis when ``squeeze``."""
    if mask is None:
        return None
    B, C, T, F = shape
    mask = mask[None] if squeeze else mask
    want = (B, C, T, F) if reduce else (B, T, F)
    if tuple(mask.shape) != want:
        raise ValueError(f'{name}: a mask of shape {want[1:] if squeeze else want} for this observation and channel_reduce, '
                         f'got {tuple(mask.shape[1:] if squeeze else mask.shape)}')
    return mask.contiguous()


def _frames(name, frames, B):
    if frames is None:
        return None
    if frames.dtype != torch.int32:
        raise NotImplementedError(f'{name}: frames int32 only, got {frames.dtype}')
    if tuple(frames.shape) != (B,):
        raise ValueError(f'{name}: frames [{B}], got {tuple(frames.shape)}')
    return frames.contiguous()


def _reduce_flag(name, channel_reduce):
    if channel_reduce not in ('median', None):
        raise ValueError(f'{name}: channel_reduce \'median\' or None, got {channel_reduce!r}')
    return channel_reduce == 'median'


def get_power_spectral_density_matrix(observation, mask=None, *, frames=None, channel_reduce='median', normalize=True):
    name = 'get_power_spectral_density_matrix'
    reduce = _reduce_flag(name, channel_reduce)
    _check(name, (torch.complex64, torch.float32), observation, mask)
    Y, squeeze = _spectrum(name, observation)
    mask = _mask(name, mask, Y.shape, squeeze, reduce)
    frames = _frames(name, frames, Y.shape[0])
    _lib.require_gpu(Y, mask, frames)
    psd = torch.ops.ptmi.bf_psd(Y, mask, None, frames, bool(normalize))[0]
    return psd[0] if squeeze else psd


def get_mvdr_vector_souden(target_psd_matrix, noise_psd_matrix, ref_channel=None, *, return_ref_channel=False):
    name = 'get_mvdr_vector_souden'
    _check(name, (torch.complex128, torch.complex128), target_psd_matrix, noise_psd_matrix)
    s, n = target_psd_matrix, noise_psd_matrix
    if s.dim() not in (3, 4) or s.shape != n.shape or s.shape[-1] != s.shape[-2] or s.numel() == 0:
        raise ValueError(f'{name}: two [B, F, C, C] or [F, C, C] matrices, got {tuple(s.shape)}, {tuple(n.shape)}')
    squeeze = s.dim() == 3
    C = s.shape[-1]
    _channels(name, C)
    if ref_channel is not None and not 0 <= int(ref_channel) < C:
        raise ValueError(f'{name}: ref_channel in [0, {C}), got {ref_channel}')
    s, n = (s[None], n[None]) if squeeze else (s, n)
    _lib.require_gpu(s, n)
    w, _, ref = torch.ops.ptmi.bf_souden(s.contiguous(), n.contiguous(), -1 if ref_channel is None else int(ref_channel))
    w = w[0] if squeeze else w
    return (w, ref) if return_ref_channel else w


def apply_beamforming_vector(vector, mix, *, frames=None):
    name = 'apply_beamforming_vector'
    _check(name, (torch.complex64, torch.complex64), vector, mix)
    X, squeeze = _spectrum(name, mix)
    vector = vector[None] if squeeze and vector.dim() == 2 else vector
    B, C, T, F = X.shape
    if tuple(vector.shape) != (B, F, C):
        raise ValueError(f'{name}: a vector [{B}, {F}, {C}] for this mix, got {tuple(vector.shape)}')
    frames = _frames(name, frames, B)
    _lib.require_gpu(vector, X, frames)
    Z = torch.ops.ptmi.bf_apply(vector.contiguous(), X, frames)
    return Z[0] if squeeze else Z


def beamforming_vector(observation, speech_mask, noise_mask, *, frames=None, ref_channel=None, channel_reduce='median'):
    """The Souden MVDR vector of ``mask_beamforming``: both PSD matrices from one ``bf_psd`` launch -> ``(w [B, F, C], Y, frames,
    squeeze)`` with the checked, batched (``[B, C, T, F]``) observation ``Y`` and whether the batch axis was added."""
    name = 'mask_beamforming'
    reduce = _reduce_flag(name, channel_reduce)
    _check(name, (torch.complex64, torch.float32, torch.float32), observation, speech_mask, noise_mask)
    Y, squeeze = _spectrum(name, observation)
    if speech_mask is None or noise_mask is None:
        raise ValueError(f'{name}: a speech and a noise mask')
    speech_mask, noise_mask = (_mask(name, m, Y.shape, squeeze, reduce) for m in (speech_mask, noise_mask))
    C = Y.shape[1]
    if ref_channel is not None and not 0 <= int(ref_channel) < C:
        raise ValueError(f'{name}: ref_channel in [0, {C}), got {ref_channel}')
    frames = _frames(name, frames, Y.shape[0])
    _lib.require_gpu(Y, speech_mask, noise_mask, frames)
    psd = torch.ops.ptmi.bf_psd(Y, speech_mask, noise_mask, frames, True)
    w, _, _ = torch.ops.ptmi.bf_souden(psd[0], psd[1], -1 if ref_channel is None else int(ref_channel))
    return w, Y, frames, squeeze


def mask_beamforming(observation, speech_mask, noise_mask, *, frames=None, ref_channel=None):
    w, Y, frames, squeeze = beamforming_vector(observation, speech_mask, noise_mask, frames=frames, ref_channel=ref_channel)
    Z = torch.ops.ptmi.bf_apply(w, Y, frames)
    return Z[0] if squeeze else Z
