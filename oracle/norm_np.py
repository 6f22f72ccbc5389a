"""numpy restatement of the masked normalisation.  ORACLE - test infrastructure only.

Follows ``padertorch/modules/normalization.py``: ``mask_and_compute_stats`` (``:497-512``),
``_Normalize.forward`` (``:345-372``) and the running-statistics bookkeeping of ``Normalization``
(``_update_running_stats`` ``:204-216``, ``running_var`` ``:160-169``, ``_running_norm`` ``:233-246``).
The reference's own test (``tests/test_modules/test_norm.py:8-35``, ``normalize_ref``) states the
same forward.  The backward (``normalize_backward``, ``running_norm_backward``) is the closed form of
the derivative, written from the mathematics; the goldens (reference autograd) and torch's float64
autograd of the forward pin it in ``tests/test_oracle_norm.py``.

Every function computes in ``dtype`` (float64 unless asked otherwise): the float32 run of the same
restatement is what the GPU tests derive their tolerances from.
"""
import numpy as np


def compute_mask(shape, sequence_lengths, batch_axis, sequence_axis, dtype=np.float64):
    """``ops/sequence/mask.py:4-73``."""
    if sequence_lengths is None:
        return np.ones(shape, dtype)
    nd = len(shape)
    b, t = batch_axis % nd, sequence_axis % nd
    sb = [1] * nd
    sb[b] = -1
    st = [1] * nd
    st[t] = -1
    idx = np.arange(shape[t]).reshape(st)
    return np.broadcast_to((idx < np.asarray(sequence_lengths).reshape(sb)).astype(dtype), shape)


def _opt(a, dtype):
    return None if a is None else np.asarray(a, dtype)


def _statistics(x, statistics_axis, batch_axis, sequence_axis, sequence_lengths, shift, dtype):
    """What forward and backward share: ``(axes, mask, xm, denom, mean, power, n_values, power_scale)``."""
    axes = tuple(a % x.ndim for a in statistics_axis)
    mask = compute_mask(x.shape, sequence_lengths, batch_axis, sequence_axis, dtype)
    n_values = mask.sum(axis=axes, keepdims=True)
    xm = x * mask
    denom = np.maximum(n_values, 1)
    mean = xm.sum(axis=axes, keepdims=True) / denom
    power = (xm ** 2).sum(axis=axes, keepdims=True) / denom
    power_scale = np.maximum(power - mean ** 2 if shift else power, 0)
    return axes, mask, xm, denom, mean, power, n_values, power_scale


def normalize(x, gamma, beta, statistics_axis, batch_axis, sequence_axis, sequence_lengths, shift, scale, eps,
              dtype=np.float64):
    """``(y, mean, power, n_values)`` in ``dtype``."""
    x = np.asarray(x, dtype)
    _, mask, xm, _, mean, power, n_values, power_scale = _statistics(x, statistics_axis, batch_axis, sequence_axis,
                                                                     sequence_lengths, shift, dtype)
    y = xm
    if shift:
        y = y - mean
    if scale:
        y = y / np.sqrt(power_scale + dtype(eps))
    if gamma is not None:
        y = y * np.asarray(gamma, dtype)
    if beta is not None:
        y = y + np.asarray(beta, dtype)
    return y * mask, mean, power, n_values


def _sum_to(a, shape):
    """Sum ``a`` over the axes along which an array of ``shape`` was broadcast."""
    return a.sum(axis=tuple(d for d, s in enumerate(shape) if s == 1 and a.shape[d] != 1), keepdims=True)


def normalize_backward(gy, x, gamma, beta, statistics_axis, batch_axis, sequence_axis, sequence_lengths, shift, scale,
                       eps, dtype=np.float64):
    """``(grad_x, grad_gamma, grad_beta)`` of ``sum(gy * y)`` for the ``y`` of ``normalize`` (``None`` for an absent
    parameter).  No gradient flows through the returned statistics and the clamps pass no correction.

    With ``m`` the mask, ``g = m gy gamma``, ``c = m x - mean`` (``m x`` without shift), ``s = sqrt(power_scale + eps)``
    (1 without scale), ``N = max(n_values, 1)`` and sums over the statistics axes of a group::

        y      = m (gamma c / s + beta)
        grad_x = m (g / s  -  [shift] sum(g) / (s N)  -  [scale] sum(g c) c / (s^3 N))

    (``d mean / d x_i = 1 / N``, ``d power_scale / d x_i = 2 c_i / N`` with or without shift), and the parameters'
    gradients are the sums of ``m gy c / s`` and ``m gy`` over the axes they are broadcast along.
    """
    x, gy = np.asarray(x, dtype), np.asarray(gy, dtype)
    gamma, beta = _opt(gamma, dtype), _opt(beta, dtype)
    axes, mask, xm, denom, mean, _, _, power_scale = _statistics(x, statistics_axis, batch_axis, sequence_axis,
                                                                 sequence_lengths, shift, dtype)
    g = gy * mask
    ghat = g if gamma is None else g * gamma
    c = xm - mean if shift else xm
    s = np.sqrt(power_scale + dtype(eps)) if scale else np.ones_like(denom)
    grad_x = ghat / s
    if shift:
        grad_x = grad_x - ghat.sum(axis=axes, keepdims=True) / (s * denom)
    if scale:
        grad_x = grad_x - (ghat * c).sum(axis=axes, keepdims=True) * c / (s ** 3 * denom)
    grad_gamma = None if gamma is None else _sum_to(g * (c / s), gamma.shape)
    grad_beta = None if beta is None else _sum_to(g, beta.shape)
    return grad_x * mask, grad_gamma, grad_beta


def update_running_stats(state, mean, power, n_values, momentum, shift=True, scale=True, dtype=np.float64):
    """``Normalization._update_running_stats``; ``state`` = dict(num_tracked_values, running_mean, running_power)."""
    state = {k: (None if v is None else np.array(v, dtype)) for k, v in state.items()}
    mean, power, n_values = np.asarray(mean, dtype), np.asarray(power, dtype), np.asarray(n_values, dtype)
    state['num_tracked_values'] = state['num_tracked_values'] + n_values
    m = 1 - n_values / state['num_tracked_values'] if momentum is None else dtype(momentum)
    if shift:
        state['running_mean'] = state['running_mean'] * m + (1 - m) * mean
    if scale:
        state['running_power'] = state['running_power'] * m + (1 - m) * power
    return state


def running_var(state, eps, shift=True):
    n = np.maximum(state['num_tracked_values'], 2)
    v = state['running_power']
    if shift:
        v = n / (n - 1) * v - state['running_mean'] ** 2
    return np.maximum(v, 0) + v.dtype.type(eps)


def running_norm(x, state, gamma, beta, batch_axis, sequence_axis, sequence_lengths, shift, scale, eps,
                 dtype=np.float64):
    x = np.asarray(x, dtype)
    state = {k: _opt(v, dtype) for k, v in state.items()}
    if shift:
        x = x - state['running_mean']
    if scale:
        x = x / np.sqrt(running_var(state, eps, shift) + dtype(eps))
    if gamma is not None:
        x = x * np.asarray(gamma, dtype)
    if beta is not None:
        x = x + np.asarray(beta, dtype)
    return x * compute_mask(x.shape, sequence_lengths, batch_axis, sequence_axis, dtype)


def running_norm_backward(gy, x, state, gamma, beta, batch_axis, sequence_axis, sequence_lengths, shift, scale, eps,
                          dtype=np.float64):
    """``(grad_x, grad_gamma, grad_beta)`` of ``sum(gy * running_norm(x, ...))``: the statistics are constants, so
    ``grad_x = m gy gamma / s`` and the parameters' gradients are the sums of ``m gy (x - mean) / s`` and ``m gy``."""
    x, gy = np.asarray(x, dtype), np.asarray(gy, dtype)
    gamma, beta = _opt(gamma, dtype), _opt(beta, dtype)
    state = {k: _opt(v, dtype) for k, v in state.items()}
    g = gy * compute_mask(x.shape, sequence_lengths, batch_axis, sequence_axis, dtype)
    c = x - state['running_mean'] if shift else x
    s = np.sqrt(running_var(state, eps, shift) + dtype(eps)) if scale else dtype(1)
    grad_x = (g if gamma is None else g * gamma) / s
    grad_gamma = None if gamma is None else _sum_to(g * (c / s), gamma.shape)
    grad_beta = None if beta is None else _sum_to(g, beta.shape)
    return grad_x, grad_gamma, grad_beta


def unit_norm(x, eps=1e-12):
    """``torch.nn.functional.normalize(x, p=2, dim=-2, eps)`` as used on the deep-clustering embedding
    (padertorch/contrib/tcl/dc.py:70): x / max(||x||_2 over axis -2, eps)."""
    x = np.asarray(x)
    n = np.sqrt((x.astype(np.float64) ** 2).sum(-2, keepdims=True))
    return (x / np.maximum(n, eps)).astype(x.dtype)


def unit_norm_backward(gy, x, eps=1e-12):
    """d/dx of ``sum(gy * unit_norm(x))`` (autograd of normalize: the clamp passes no gradient)."""
    x64, g64 = np.asarray(x, np.float64), np.asarray(gy, np.float64)
    n = np.sqrt((x64 ** 2).sum(-2, keepdims=True))
    d = np.maximum(n, eps)
    y = x64 / d
    proj = (g64 * y).sum(-2, keepdims=True) * np.where(n > eps, 1.0, 0.0)
    return ((g64 - y * proj) / d).astype(np.asarray(x).dtype)
