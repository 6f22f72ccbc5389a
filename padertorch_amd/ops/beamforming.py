"""Mask-based beamforming (Souden MVDR, GEV and PCA vectors, blind analytic normalization, phase correction) on the HIP kernels of
``csrc/beamform.hip``: what a speech and a noise mask are estimated for
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
    get_gev_vector(target_psd_matrix, noise_psd_matrix, *, return_eigenvalue=False)
        the principal generalized eigenvector of ``(Phi_s, Phi_n)`` per bin (``pb_bss.extraction.get_bf_vector('gev', ...)``), all in
        float64: Cholesky ``Phi_n = L L^H``; ``A = L^-1 Phi_s L^-H`` by two triangular solves (no inverse), made exactly Hermitian
        (``(A + A^H) / 2``); cyclic complex Jacobi on ``A``, a sweep while ``off(A)^2 > (2^-52)^2 ||A||_F^2``, at most 16 sweeps;
        ``v`` the eigenvector of the largest eigenvalue ``lambda`` (first maximum); ``w = L^-H v``, so ``w^H Phi_n w = 1``
        (``scipy.linalg.eigh(a, b)``'s normalisation) -> ``[B, F, C]`` complex64.  Gauge: ``w`` is rotated so that its component of
        largest squared magnitude (first maximum, compared in float64) is real and positive.  A bin whose Cholesky meets a pivot that
        is not ``> 0`` (a zero or indefinite ``Phi_n``, NaN) gives ``w = 0`` and ``lambda = 0`` - the Souden kernel's "all-zero
        ``Phi_n`` gives a zero output" - and so does an all-zero ``Phi_s``.  ``return_eigenvalue`` also returns ``lambda`` as
        ``[B, F]`` float64.
    get_pca_vector(target_psd_matrix, *, return_eigenvalue=False)
        the same Jacobi on ``Phi_s`` alone: the principal eigenvector with unit 2-norm, same gauge; an all-zero matrix gives ``w = 0``.
    blind_analytic_normalization(vector, noise_psd_matrix)
        ``w sqrt(|w^H Phi_n Phi_n w|) / max(|w^H Phi_n w|, tiny)`` in float64 on the complex64 vector; a zero vector stays zero.
    phase_correction(vector)
        per example, for ``f = 1 .. F-1`` in order: ``w'_f = w_f exp(-i arg(sum_c w_f,c conj(w'_{f-1},c)))``; a sum that is exactly
        zero rotates by nothing.  Every step is a unit rotation, ``w'_f = c_f w_f`` with ``c_0 = 1``,
        ``c_f = c_{f-1} conj(d_f / |d_f|)`` and ``d_f = sum_c w_f,c conj(w_{f-1},c)`` on the uncorrected vectors (``c_f = 1`` where
        ``d_f = 0``): the kernel computes the ``c_f`` as a parallel scan of float64 phasors in one fixed order (two runs agree bit
        for bit).  It is defined on the stored complex64 vector, so this function and ``mask_beamforming`` give the same bits.
    get_bf_vector(beamformer, target_psd_matrix, noise_psd_matrix, *, ref_channel=None)
        ``pb_bss.extraction.get_bf_vector``: ``beamformer`` one of ``BEAMFORMERS`` (``'mvdr_souden'``, ``'gev'``, ``'pca'``, each
        optionally with ``'+ban'``: the vector goes through ``blind_analytic_normalization``); ``ref_channel`` is for
        ``mvdr_souden`` only; any other name raises ``ValueError``.  No phase correction, as upstream.
    mask_beamforming(observation, speech_mask, noise_mask, *, frames=None, ref_channel=None, beamformer='mvdr_souden')
        PSD matrices, vector and application together -> ``Z [B, T, F]``: both PSD matrices from ONE pass over the observation, then
        for ``mvdr_souden`` the solve and the reference-channel stage, for ``gev*`` / ``pca*`` ONE eigen launch (BAN inside) and
        one ``phase_correction`` launch - without it the phase of every bin is the gauge's artefact and the iSTFT of the output
        means nothing -, then the apply pass.

Inference only: an input that requires grad raises.  complex64 / float32 (PSD matrices complex128) on the GPU only: other dtypes
raise ``NotImplementedError``, CPU tensors the "no CPU fallback" error; more than 8 channels raise ``NotImplementedError``.
"""
import torch

from .. import _lib
from . import library  # noqa: F401  (registers torch.ops.ptmi.*)

__all__ = ['get_power_spectral_density_matrix', 'get_mvdr_vector_souden', 'apply_beamforming_vector', 'mask_beamforming',
           'get_gev_vector', 'get_pca_vector', 'blind_analytic_normalization', 'phase_correction', 'get_bf_vector', 'BEAMFORMERS',
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


BEAMFORMERS = ('mvdr_souden', 'gev', 'pca', 'mvdr_souden+ban', 'gev+ban', 'pca+ban')


def parse_beamformer(name, beamformer, ref_channel=None):
    """``'gev+ban'`` -> ``('gev', True)``; any name but ``BEAMFORMERS`` raises, and so does a reference channel for another vector
    than the Souden one."""
    if beamformer not in BEAMFORMERS:
        raise ValueError(f'{name}: beamformer one of {", ".join(map(repr, BEAMFORMERS))}, got {beamformer!r}')
    kind, _, ban = beamformer.partition('+')
    if kind != 'mvdr_souden' and ref_channel is not None:
        raise ValueError(f'{name}: ref_channel is for mvdr_souden only, got {ref_channel} for {beamformer!r}')
    return kind, bool(ban)


def _psd_matrices(name, *matrices):
    """Checked ``[B, F, C, C]`` or ``[F, C, C]`` complex128 matrices of one shape -> contiguous ``[B, F, C, C]`` ones and whether the
    batch axis was added."""
    _check(name, (torch.complex128,) * len(matrices), *matrices)
    s = matrices[0]
    if s.dim() not in (3, 4) or any(m.shape != s.shape for m in matrices) or s.shape[-1] != s.shape[-2] or s.numel() == 0:
        raise ValueError(f'{name}: [B, F, C, C] or [F, C, C] matrices of one shape, got '
                         + ', '.join(str(tuple(m.shape)) for m in matrices))
    _channels(name, s.shape[-1])
    squeeze = s.dim() == 3
    return [(m[None] if squeeze else m).contiguous() for m in matrices], squeeze


def _vector(name, vector, psd=None):
    """A checked ``[B, F, C]`` or ``[F, C]`` complex64 vector (for the matrices ``psd``, when given) -> contiguous ``[B, F, C]`` and
    whether the batch axis was added."""
    if vector.dim() not in (2, 3) or vector.numel() == 0:
        raise ValueError(f'{name}: a vector [B, F, C] or [F, C], got {tuple(vector.shape)}')
    _channels(name, vector.shape[-1])
    if psd is not None and tuple(psd.shape) != (*vector.shape, vector.shape[-1]):
        raise ValueError(f'{name}: a noise PSD matrix {(*vector.shape, vector.shape[-1])} for this vector, got {tuple(psd.shape)}')
    squeeze = vector.dim() == 2
    return (vector[None] if squeeze else vector).contiguous(), squeeze


def _eig(name, target, noise, gev, ban, return_eigenvalue):
    matrices, squeeze = _psd_matrices(name, *(m for m in (target, noise) if m is not None))
    _lib.require_gpu(*matrices)
    w, lam, _ = torch.ops.ptmi.bf_eig(matrices[0], matrices[1] if noise is not None else None, gev, ban)
    w, lam = (w[0], lam[0]) if squeeze else (w, lam)
    return (w, lam) if return_eigenvalue else w


def get_gev_vector(target_psd_matrix, noise_psd_matrix, *, return_eigenvalue=False):
    return _eig('get_gev_vector', target_psd_matrix, noise_psd_matrix, True, False, return_eigenvalue)


def get_pca_vector(target_psd_matrix, *, return_eigenvalue=False):
    return _eig('get_pca_vector', target_psd_matrix, None, False, False, return_eigenvalue)


def blind_analytic_normalization(vector, noise_psd_matrix):
    name = 'blind_analytic_normalization'
    _check(name, (torch.complex64, torch.complex128), vector, noise_psd_matrix)
    w, squeeze = _vector(name, vector, noise_psd_matrix)
    _lib.require_gpu(w, noise_psd_matrix)
    out = torch.ops.ptmi.bf_ban(w, (noise_psd_matrix[None] if squeeze else noise_psd_matrix).contiguous())
    return out[0] if squeeze else out


def phase_correction(vector):
    name = 'phase_correction'
    _check(name, (torch.complex64,), vector)
    w, squeeze = _vector(name, vector)
    _lib.require_gpu(w)
    out = torch.ops.ptmi.bf_phase(w)
    return out[0] if squeeze else out


def _bf_vector(kind, ban, target, noise, ref_channel):
    """The vector of a checked, batched pair of PSD matrices: one launch for ``gev`` / ``pca`` (BAN inside), the Souden stages and
    the stand-alone BAN launch for ``mvdr_souden``."""
    if kind == 'mvdr_souden':
        w, _, _ = torch.ops.ptmi.bf_souden(target, noise, -1 if ref_channel is None else int(ref_channel))
        return torch.ops.ptmi.bf_ban(w, noise) if ban else w
    return torch.ops.ptmi.bf_eig(target, noise if kind == 'gev' or ban else None, kind == 'gev', ban)[0]


def get_bf_vector(beamformer, target_psd_matrix, noise_psd_matrix, *, ref_channel=None):
    name = 'get_bf_vector'
    kind, ban = parse_beamformer(name, beamformer, ref_channel)
    (s, n), squeeze = _psd_matrices(name, target_psd_matrix, noise_psd_matrix)
    if ref_channel is not None and not 0 <= int(ref_channel) < s.shape[-1]:
        raise ValueError(f'{name}: ref_channel in [0, {s.shape[-1]}), got {ref_channel}')
    _lib.require_gpu(s, n)
    w = _bf_vector(kind, ban, s, n, ref_channel)
    return w[0] if squeeze else w


def beamforming_vector(observation, speech_mask, noise_mask, *, frames=None, ref_channel=None, channel_reduce='median',
                       beamformer='mvdr_souden'):
    """The vector of ``mask_beamforming`` WITHOUT the phase correction: both PSD matrices from one ``bf_psd`` launch ->
    ``(w [B, F, C], Y, frames, squeeze)`` with the checked, batched (``[B, C, T, F]``) observation ``Y`` and whether the batch axis
    was added."""
    name = 'mask_beamforming'
    kind, ban = parse_beamformer(name, beamformer, ref_channel)
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
    return _bf_vector(kind, ban, psd[0], psd[1], ref_channel), Y, frames, squeeze


def mask_beamforming(observation, speech_mask, noise_mask, *, frames=None, ref_channel=None, beamformer='mvdr_souden'):
    w, Y, frames, squeeze = beamforming_vector(observation, speech_mask, noise_mask, frames=frames, ref_channel=ref_channel,
                                               beamformer=beamformer)
    if not beamformer.startswith('mvdr_souden'):
        w = torch.ops.ptmi.bf_phase(w)
    Z = torch.ops.ptmi.bf_apply(w, Y, frames)
    return Z[0] if squeeze else Z
