"""Launchers of the three feature kernels of ``csrc/je_features.hip`` (``include/ptmi.h``: ``ptmi_je_logmel_front``,
``ptmi_je_feature_shape``, ``ptmi_je_feature_tail``) behind ``contrib/je/modules/features.py`` and ``contrib/je/modules/augment.py``.

Every random quantity is a HOST array here (drawn by the modules in the reference's order); this file turns it into a small device table
through the pinned staging buffer and launches.  float32, forward only, no CPU fallback.
"""
from ctypes import c_float, c_int32

import numpy as np
import torch

from .. import _lib

__all__ = ['front_tile', 'shape_tile', 'logmel_front', 'feature_shape', 'feature_tail', 'lengths_as_frames']

MAX_F, MAX_M, MAX_C, MAX_K, DELTA_WIDTH = 1025, 256, 8, 9, 5


def front_tile():
    """Frames of a workgroup's tile in ``logmel_front``."""
    return int(_lib.load().ptmi_je_front_tile())


def shape_tile():
    """Output frames of a workgroup's tile in ``feature_shape``."""
    return int(_lib.load().ptmi_je_shape_tile())


def lengths_as_frames(seq_len):
    """``compute_mask``'s ``index < torch.Tensor(length).long()`` as a frame count: a fractional length (time warping returns them) is
    truncated, as the reference's masks truncate it (``ops/sequence/mask.py:64``)."""
    return None if seq_len is None else np.asarray(seq_len, dtype=np.float32).astype(np.int64)


def _table(values, dtype, device):
    return None if values is None else _lib.host_to_device(np.ascontiguousarray(values), dtype, device)


def _features(x, what):
    _lib.require_gpu(x)
    if x.dtype != torch.float32 or x.dim() != 4:
        raise NotImplementedError(f'{what}: a float32 [B, C, M, T] tensor, got {x.dtype} {tuple(x.shape)}')
    if x.shape[1] > 3 * MAX_C or x.shape[2] > MAX_M:
        raise NotImplementedError(f'{what}: at most C = {MAX_C} channels (x 3 with deltas) and M = {MAX_M} bands, got {tuple(x.shape)}')
    x = x.contiguous()
    return x if x.data_ptr() % 16 == 0 else x.clone()


def logmel_front(x, bands, max_bin=None, pairs=(), *, edges_hz=None, bin_hz=None, gain=None, partner=None, partner_gain=None,
                 lam=None, eps=1e-12):
    """Stacked STFT ``[B, C, T, F, 2]`` (or complex64 ``[B, C, T, F]``) -> ``(logmel [B, C, M, T], ipd_cos, ipd_sin)``.

    ``bands``: the ``_Bands`` of the static, normalised filterbank; ``edges_hz [B, M + 2]`` (host, strictly increasing rows) replaces it
    by per-example triangles evaluated at ``k * bin_hz``.  ``gain [B]``, ``partner [B]`` (example index), ``partner_gain [B]``,
    ``lam [B]``: ``z = gain x_b + lam partner_gain x_partner(b)`` before the square.  ``pairs``: ``((ref, other), ...)`` channel pairs
    whose phase difference at bin ``max_bin[m]`` comes back as ``ipd_cos`` / ``ipd_sin [B, P, M, T]`` (``None`` without pairs).
    """
    _lib.require_gpu(x)
    if x.is_complex():
        x = torch.view_as_real(x)
    if x.dtype != torch.float32 or x.dim() != 5 or x.shape[-1] != 2:
        raise NotImplementedError(f'logmel_front: a float32 [B, C, T, F, 2] or complex64 [B, C, T, F] tensor, got {x.dtype} {tuple(x.shape)}')
    B, C, T, F = x.shape[:4]
    M = bands.M
    if F > MAX_F or M > MAX_M or C > MAX_C:
        raise NotImplementedError(f'logmel_front covers F <= {MAX_F} bins (STFT sizes up to {2 * MAX_F - 2}), M <= {MAX_M} filters and '
                                  f'C <= {MAX_C} channels, got F = {F}, M = {M}, C = {C}')
    assert F == bands.F, (F, bands.F)
    x = x.contiguous()
    if x.data_ptr() % 8:
        x = x.clone()
    dev = x.device
    tb = bands.get(dev)
    if edges_hz is not None:
        edges_hz = np.asarray(edges_hz, dtype=np.float32)
        assert edges_hz.shape == (B, M + 2), (edges_hz.shape, (B, M + 2))
        assert np.isfinite(edges_hz).all() and (np.diff(edges_hz, axis=-1) > 0).all(), 'filter edges must increase strictly'
        assert bin_hz is not None and bin_hz > 0, bin_hz
    if partner is not None:
        partner = np.asarray(partner)
        assert partner.shape == (B,) and ((0 <= partner) & (partner < B)).all(), partner
        partner_gain = np.ones(B) if partner_gain is None else partner_gain
    pairs = [tuple(p) for p in pairs]
    assert all(len(p) == 2 and 0 <= min(p) and max(p) < C for p in pairs), (pairs, C)
    P = len(pairs)
    logmel = torch.empty((B, C, M, T), dtype=torch.float32, device=dev)
    cos = torch.empty((B, P, M, T), dtype=torch.float32, device=dev) if P else None
    sin = torch.empty_like(cos) if P else None
    if P:
        max_bin = np.asarray(max_bin)
        assert max_bin.shape == (M,) and ((0 <= max_bin) & (max_bin < F)).all(), max_bin
    if B and T:
        # (the tables stay referenced until the launch is enqueued: a freed block would be handed to the next table)
        d_gain, d_partner, d_edges = _table(gain, torch.float32, dev), _table(partner, torch.int32, dev), _table(edges_hz, torch.float32, dev)
        d_pgain = _table(partner_gain if partner is not None else None, torch.float32, dev)
        d_lam = _table(lam if partner is not None else None, torch.float32, dev)
        d_bin = _table(max_bin if P else None, torch.int32, dev)
        _lib.call('ptmi_je_logmel_front', x.data_ptr(), B, C, T, F, _lib.ptr(d_gain), _lib.ptr(d_partner), _lib.ptr(d_pgain), _lib.ptr(d_lam),
                  tb['lo'].data_ptr(), tb['cnt'].data_ptr(), tb['off'].data_ptr(), tb['w'].data_ptr(), _lib.ptr(d_edges),
                  float(bin_hz) if edges_hz is not None else 0., _lib.ptr(d_bin), M,
                  (c_int32 * max(P, 1))(*[p[0] for p in pairs]), (c_int32 * max(P, 1))(*[p[1] for p in pairs]), P, float(eps),
                  logmel.data_ptr(), _lib.ptr(cos), _lib.ptr(sin), _lib.stream(dev), timer='je_logmel_front')
    return logmel, cos, sin


def feature_shape(x, *, time_indices=None, taps=None, delta_kernel=None, delta_delta_kernel=None, seq_len=None):
    """``[B, C, M, T]`` -> ``[B, C (1 + d + dd), M, T']``: time warp (``time_indices [B, T']``, host float64, in ``[0, T - 1]``), the
    separable blur ``taps [B, k]`` over the reflect-padded plane, then the static channels followed by their correlations with the width-5
    ``delta_kernel`` / ``delta_delta_kernel`` (zero in the two frames at either edge and from ``seq_len - 2`` on).  Nothing to do: ``x``."""
    x = _features(x, 'feature_shape')
    if time_indices is None and taps is None and delta_kernel is None and delta_delta_kernel is None:
        return x
    B, C, M, T = x.shape
    dev = x.device
    if C > MAX_C:
        raise NotImplementedError(f'feature_shape covers C <= {MAX_C} channels, got {C}')
    To, floor_, frac = T, None, None
    if time_indices is not None:
        tau = np.asarray(time_indices, dtype=np.float64)
        assert tau.ndim == 2 and tau.shape[0] == B, (tau.shape, B)
        assert T > 0 and (tau >= 0).all() and (tau <= T - 1).all(), 'time indices outside [0, T - 1]'
        To = tau.shape[1]
        floor_ = np.floor(tau)
        frac = (tau - floor_).astype(np.float32)                  # the ceil weight 1 - ceil + tau; the floor weight is 1 - frac
        floor_ = floor_.astype(np.int32)
    k = 1
    if taps is not None:
        taps = np.asarray(taps.cpu() if torch.is_tensor(taps) else taps, dtype=np.float32)
        assert taps.ndim == 2 and taps.shape[0] == B, (taps.shape, B)
        k = taps.shape[1]
        if k % 2 == 0 or k > MAX_K:
            raise NotImplementedError(f'feature_shape covers odd blur kernels of k <= {MAX_K} taps, got k = {k}')
        if min(To, M) < (k + 1) // 2:
            raise NotImplementedError(f'a reflect-padded blur of k = {k} taps needs T and M >= (k + 1) / 2 = {(k + 1) // 2}, got T = {To}, M = {M}')
    kernels = []
    for kern in (delta_kernel, delta_delta_kernel):
        if kern is not None:
            kern = np.asarray(kern.cpu() if torch.is_tensor(kern) else kern, dtype=np.float32).reshape(-1)
            if len(kern) != DELTA_WIDTH:
                raise NotImplementedError(f'feature_shape covers delta kernels of width {DELTA_WIDTH}, got width {len(kern)}')
            kern = (c_float * DELTA_WIDTH)(*kern.tolist())
        kernels.append(kern)
    n_out = C * (1 + (delta_kernel is not None) + (delta_delta_kernel is not None))
    out = torch.empty((B, n_out, M, To), dtype=torch.float32, device=dev)
    if B and To:
        d_floor, d_frac, d_taps = _table(floor_, torch.int32, dev), _table(frac, torch.float32, dev), _table(taps, torch.float32, dev)
        d_len = _table(lengths_as_frames(seq_len), torch.int32, dev)
        _lib.call('ptmi_je_feature_shape', x.data_ptr(), B, C, M, T, _lib.ptr(d_floor), _lib.ptr(d_frac), To, _lib.ptr(d_taps), k,
                  int(delta_kernel is not None), int(delta_delta_kernel is not None), kernels[0], kernels[1], DELTA_WIDTH, _lib.ptr(d_len),
                  out.data_ptr(), _lib.stream(dev), timer='je_feature_shape')
    return out


def _stat(t, C, M, name):
    """A statistics tensor ``[1, C | 1, M | 1, 1]`` as (contiguous float32 tensor, stride over c, stride over f)."""
    if t is None:
        return None, 0, 0
    assert t.dim() == 4 and t.shape[0] == 1 and t.shape[3] == 1 and t.shape[1] in (1, C) and t.shape[2] in (1, M), (name, tuple(t.shape))
    t = t.detach().to(torch.float32).contiguous()
    return t, (t.shape[2] if t.shape[1] > 1 else 0), int(t.shape[2] > 1)


def _masks(tables, B, dev):
    if tables is None:
        return None, None, 0
    onset, offset = (np.asarray(t, dtype=np.int32) for t in tables)
    assert onset.ndim == 2 and onset.shape[1] == B and offset.shape == onset.shape, (onset.shape, offset.shape, B)
    return _table(onset, torch.int32, dev), _table(offset, torch.int32, dev), onset.shape[0]


def feature_tail(x, *, mean=None, rstd=None, clamp=None, ipd_cos=None, ipd_sin=None, partner=None, lam=None, noise_scale=None, noise=None,
                 time_masks=None, freq_masks=None, seq_len=None):
    """``[B, C, M, T]`` -> ``[B, C + 2 P, M, T]`` in one pass: ``clamp((x - mean) rstd)`` masked by ``t < seq_len`` on the feature
    channels (``mean`` / ``rstd``: device tensors ``[1, C | 1, M | 1, 1]``), the ``ipd_cos`` / ``ipd_sin [B, P, M, T]`` planes appended,
    mixup ``lam v_b + (1 - lam) v_partner(b)``, ``+ noise_scale_b noise`` and the ``(onset, offset)`` tables ``[n, B]`` of time and
    frequency masks (host arrays).  Every stage whose argument is ``None`` is off."""
    x = _features(x, 'feature_tail')
    B, C, M, T = x.shape
    dev = x.device
    P = 0
    if ipd_cos is not None:
        ipd_cos, ipd_sin = _features(ipd_cos, 'feature_tail'), _features(ipd_sin, 'feature_tail')
        P = ipd_cos.shape[1]
        assert ipd_cos.shape == ipd_sin.shape == (B, P, M, T), (ipd_cos.shape, ipd_sin.shape, x.shape)
    mean, sc, sf = _stat(mean, C, M, 'mean')
    rstd, sc_, sf_ = _stat(rstd, C, M, 'rstd')
    assert mean is None or rstd is None or (sc, sf) == (sc_, sf_), 'mean and rstd of different shapes'
    sc, sf = (sc, sf) if mean is not None else (sc_, sf_)
    if partner is not None:
        partner, lam = np.asarray(partner), np.asarray(lam, dtype=np.float32)
        assert partner.shape == lam.shape == (B,) and ((0 <= partner) & (partner < B)).all() and ((0 <= lam) & (lam <= 1)).all(), (partner, lam)
    out = torch.empty((B, C + 2 * P, M, T), dtype=torch.float32, device=dev)
    if noise is not None:
        _lib.require_gpu(noise)
        assert noise.shape == out.shape and noise.dtype == torch.float32, (noise.shape, out.shape)
        noise = noise.contiguous()
    t_on, t_off, n_t = _masks(time_masks, B, dev)
    f_on, f_off, n_f = _masks(freq_masks, B, dev)
    if B and T:
        d_partner, d_lam = _table(partner, torch.int32, dev), _table(lam if partner is not None else None, torch.float32, dev)
        d_scale = _table(noise_scale if noise is not None else None, torch.float32, dev)
        d_len = _table(lengths_as_frames(seq_len), torch.int32, dev)
        _lib.call('ptmi_je_feature_tail', x.data_ptr(), B, C, M, T, _lib.ptr(mean), _lib.ptr(rstd), sc, sf, int(clamp is not None),
                  float(clamp or 0.), _lib.ptr(ipd_cos), _lib.ptr(ipd_sin), P, _lib.ptr(d_partner), _lib.ptr(d_lam), _lib.ptr(d_scale),
                  _lib.ptr(noise), _lib.ptr(t_on), _lib.ptr(t_off), n_t, _lib.ptr(f_on), _lib.ptr(f_off), n_f, _lib.ptr(d_len), out.data_ptr(),
                  _lib.stream(dev), timer='je_feature_tail')
    return out
