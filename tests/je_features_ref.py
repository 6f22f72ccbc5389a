"""Plain numpy restatement of the three feature kernels (``csrc/je_features.hip``), in float64 for the tests' reference and in float32
(``dt=np.float32``) to measure how far that arithmetic alone strays - the measured values behind the gates of ``test_gpu_je_features.py``.
Dense matrices and fancy indexing throughout: nothing of the kernels' tiling."""
import numpy as np


def _b(v, dt, nd=5):
    return np.asarray(v).astype(dt).reshape((-1,) + (1,) * (nd - 1))


def triangles(edges_hz, F, bin_hz, dt=np.float64):
    """``[B, M, F]``: ``max(0, min((f - l) / (c - l), (r - f) / (r - c)))`` at ``f = k bin_hz``, rows normalised by ``sum + 1e-6``."""
    e, f = np.asarray(edges_hz).astype(dt), (np.arange(F) * bin_hz).astype(dt)
    l, c, r = e[:, :-2, None], e[:, 1:-1, None], e[:, 2:, None]
    fb = np.clip(np.minimum((f - l) / (c - l), (r - f) / (r - c)), 0, None)
    return fb / (fb.sum(-1, keepdims=True) + dt(1e-6))


def front(x, fb, max_bin=None, pairs=(), gain=None, partner=None, partner_gain=None, lam=None, eps=1e-12, dt=np.float64):
    """``x [B, C, T, F, 2]``, ``fb [1 | B, M, F]`` -> ``logmel [B, C, M, T]``, ``ipd_cos``, ``ipd_sin [B, P, M, T]``."""
    x = x.astype(dt)
    z = x if gain is None else x * _b(gain, dt)
    if partner is not None:
        z = z + _b(lam, dt) * (_b(partner_gain, dt) * x[partner])
    logmel = np.log(np.einsum('bctf,bmf->bcmt', (z ** 2).sum(-1), np.broadcast_to(fb.astype(dt), (len(x),) + fb.shape[1:])) + dt(eps))
    if not pairs:
        return logmel, None, None
    re, im = z[..., max_bin, 0], z[..., max_bin, 1]
    ref, oth = (list(c) for c in zip(*pairs))
    ipd = np.arctan2(im[:, oth] * re[:, ref] - re[:, oth] * im[:, ref], re[:, oth] * re[:, ref] + im[:, oth] * im[:, ref]).swapaxes(-2, -1)
    return logmel, np.cos(ipd), np.sin(ipd)


def shape(x, tau=None, taps=None, kd=None, kdd=None, seq_len=None, dt=np.float64):
    """``x [B, C, M, T]`` -> ``[B, C (1 + d + dd), M, T']``: warp by ``tau [B, T']``, blur by ``taps [B, k]``, append the deltas."""
    x = x.astype(dt)
    B = len(x)
    if tau is not None:
        ce, fl = np.ceil(tau).astype(int), np.floor(tau).astype(int)
        cw, fw = (1 - ce + tau).astype(np.float32).astype(dt), ((1 - tau + fl) * (fl != ce)).astype(np.float32).astype(dt)
        x = np.stack([x[b][..., ce[b]] * cw[b] + x[b][..., fl[b]] * fw[b] for b in range(B)])
    M, T = x.shape[2:]
    if taps is not None:
        k = taps.shape[1]
        xp = np.pad(x, ((0, 0), (0, 0), (k // 2, k // 2), (k // 2, k // 2)), mode='reflect')
        k2 = (taps[:, :, None].astype(dt) * taps[:, None, :].astype(dt))
        x = sum(k2[:, i, j].reshape(B, 1, 1, 1) * xp[:, :, i:i + M, j:j + T] for i in range(k) for j in range(k))
    out = [x]
    for kern in (kd, kdd):
        if kern is not None:
            y = np.zeros_like(x)
            if T > 4:
                y[..., 2:T - 2] = sum(dt(kern[i]) * x[..., i:T - 4 + i] for i in range(5))
            if seq_len is not None:
                y = y * (np.arange(T) < np.asarray(seq_len).reshape(B, 1, 1, 1) - 2)
            out.append(y)
    return np.concatenate(out, 1)


def tail(x, mean=None, rstd=None, clamp=None, cos=None, sin=None, partner=None, lam=None, noise_scale=None, noise=None,
         time_masks=None, freq_masks=None, seq_len=None, dt=np.float64):
    """``x [B, C, M, T]`` -> ``[B, C + 2 P, M, T]``; ``mean`` / ``rstd`` broadcast against ``x``; mask tables ``(onset, offset) [n, B]``."""
    v = x.astype(dt)
    B, _, M, T = v.shape
    if mean is not None:
        v = v - mean.astype(dt)
    if rstd is not None:
        v = v * rstd.astype(dt)
    if clamp is not None:
        v = np.clip(v, -clamp, clamp)
    if seq_len is not None:
        v = v * (np.arange(T) < np.asarray(seq_len).reshape(B, 1, 1, 1))
    if cos is not None:
        v = np.concatenate([v, cos.astype(dt), sin.astype(dt)], 1)
    if partner is not None:
        v = _b(lam, dt, 4) * v + (1 - _b(lam, dt, 4)) * v[partner]
    if noise is not None:
        v = v + _b(noise_scale, dt, 4) * noise.astype(dt)
    for tables, idx in ((time_masks, np.arange(T).reshape(1, 1, 1, T)), (freq_masks, np.arange(M).reshape(1, 1, M, 1))):
        for on, off in zip(*(tables or ((), ()))):
            v = v * ((idx < on.reshape(B, 1, 1, 1)) | (idx >= off.reshape(B, 1, 1, 1)))
    return v
