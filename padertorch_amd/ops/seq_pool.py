"""``reverse_sequence`` (``padertorch/contrib/je/modules/rnn.py:130-154``) and the masked reductions over time of
``contrib/je/modules/reduce.py`` on the kernels of ``csrc/seq_pool.hip``.

    reverse_sequence(x [B, T, F], seq_len=None) -> [B, T, F]          one gather launch, differentiable, any input strides
    rows_layout(x [B, T, F]) -> [B, T, F] contiguous                  the same launch as a plain copy (``b f t`` views -> rows)
    seq_pool(x, seq_len, axis, mode, keepdims, alpha=None)            mode: 'sum', 'mean', 'max', 'last', 'autopool'

``seq_pool`` takes any number of dimensions with the batch on axis 0 and any ``axis >= 1``.  ``x`` is read in place as ``[B, M, T, I]``
through four strides (``M``: the axes between batch and time, ``I``: the axes behind time); only when the axes of ``M`` or of ``I``
cannot be collapsed into one stride each (a 4-D+ view with gaps) is ``x`` copied first.  Thread map: a wavefront per row when the time
axis has unit stride, else a thread per row; the backward follows the layout of the fresh contiguous ``dx``.

``seq_len``: None, a list, a numpy array, a CPU tensor or a CUDA int32 / int64 tensor (read by the kernels: nothing is read back, so a
captured graph serves other lengths); lengths are clipped to ``[0, T]``.

    sum       sum over t < len                                  no lengths: the plain sum
    mean      sum / (float(len) + 1e-6f) (reduce.py:42)         no lengths: x.mean; length 0 gives 0
    max       (values, int64 indices) like x.max(axis)          positions behind the length count as -inf; length 0: (-inf, 0)
    last      x[b, len_b - 1] along axis                        no lengths: the last position
    autopool  sum_t softmax_t(alpha x) x over t < len           alpha: a float or a tensor [C, 1] / [C] (then x is [B, C, T], axis -1);
                                                                length 0 gives NaN as in the reference

Where the reference multiplies by a 0 / 1 mask, a NaN or an infinity BEHIND the length poisons its result (``NaN * 0``); these kernels
never read behind the length, so ``sum``, ``mean`` and ``autopool`` ignore it - a departure.  ``reverse_sequence`` reproduces it: the
positions behind the length are ``x[b, (len - 1 - t) mod T] * 0``.  fp32 on the GPU only.
"""
import torch
from torch.autograd.function import once_differentiable

from .. import _lib
from . import library  # noqa: F401  (registers torch.ops.ptmi.*)
from .gru import device_lengths

__all__ = ['reverse_sequence', 'rows_layout', 'seq_pool', 'MODES']

MODES = {'sum': 0, 'mean': 1, 'max': 2, 'last': 3, 'autopool': 4}


def _check(name, *tensors):
    for t in tensors:
        if t is not None and t.dtype != torch.float32:
            raise NotImplementedError(f'{name}: float32 only, got {t.dtype}')
    _lib.require_gpu(*tensors)


class _GatherFn(torch.autograd.Function):
    """Kernel ``seq_gather``: mode 1 forward, mode 2 (plain zeros behind the length) backward; mode 0 is its own adjoint up to layout."""

    @staticmethod
    def forward(ctx, x, lengths, mode):
        ctx.save_for_backward(lengths)
        ctx.mode = mode
        return torch.ops.ptmi.seq_gather(x, lengths, mode)

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        lengths, = ctx.saved_tensors
        return torch.ops.ptmi.seq_gather(g, lengths, 2 if ctx.mode else 0), None, None


def _btf(name, x):
    _check(name, x)
    if x.dim() != 3 or x.numel() == 0:
        raise ValueError(f'{name}: x [B, T, F], got {tuple(x.shape)}')


def reverse_sequence(x, seq_len=None):
    """``out[b, t] = x[b, len_b - 1 - t]`` for ``t < len_b`` and ``x[b, (len_b - 1 - t) mod T] * 0`` behind; ``seq_len=None``: ``flip(1)``."""
    _btf('reverse_sequence', x)
    return _GatherFn.apply(x, device_lengths(seq_len, x.shape[0], x.device), 1)


def rows_layout(x):
    """``x [B, T, F]`` of any strides as a contiguous tensor, by the gather kernel."""
    _btf('rows_layout', x)
    return x if x.is_contiguous() else _GatherFn.apply(x, None, 0)


def _collapse(shape, strides):
    """One (size, stride) for the axes ``shape`` / ``strides`` (row-major order), or None when they do not collapse."""
    dims = [(n, s) for n, s in zip(shape, strides) if n != 1]
    if not dims:
        return 1, 0
    size, stride = dims[-1]
    for n, s in reversed(dims[:-1]):
        if s != size * stride:
            return None
        size *= n
    return size, stride


def geometry(x, axis):
    """``(x or its contiguous copy, dims [B, M, T, I], strides)`` for the time axis ``axis >= 1``."""
    for _ in range(2):
        mid = _collapse(x.shape[1:axis], x.stride()[1:axis])
        inner = _collapse(x.shape[axis + 1:], x.stride()[axis + 1:])
        if mid is not None and inner is not None:
            break
        x = x.contiguous()
    dims = [x.shape[0], mid[0], x.shape[axis], inner[0]]
    strides = [x.stride(0), mid[1], x.stride(axis), inner[1]]
    return x, dims, [s if n > 1 else 0 for n, s in zip(dims, strides)]


class _PoolFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, lengths, alpha, alpha0, axis, mode):
        xg, dims, strides = geometry(x, axis)
        wave = strides[2] == 1
        a = None if alpha is None else alpha.reshape(-1).contiguous()
        y, index = torch.ops.ptmi.seq_pool_forward(xg, dims, strides, lengths, mode, a, alpha0, wave)
        ctx.save_for_backward(xg, lengths, a, y if mode == 4 else None, index)
        ctx.cfg = (dims, strides, mode, alpha0, tuple(x.shape), None if alpha is None else tuple(alpha.shape))
        out_shape = x.shape[:axis] + x.shape[axis + 1:]
        y = y.view(out_shape)
        if mode == 2:
            index = index.view(out_shape)
            ctx.mark_non_differentiable(index)
            return y, index
        return y, None

    @staticmethod
    @once_differentiable
    def backward(ctx, g, _):
        x, lengths, a, y, index = ctx.saved_tensors
        dims, strides, mode, alpha0, shape, alpha_shape = ctx.cfg
        want = a is not None and ctx.needs_input_grad[2]
        dx, dalpha = torch.ops.ptmi.seq_pool_backward(x, dims, strides, lengths, mode, a, alpha0, g.contiguous(), y, index, want)
        return (dx.view(shape) if ctx.needs_input_grad[0] else None, None, dalpha.view(alpha_shape) if want else None, None, None, None)


def seq_pool(x, seq_len=None, axis=-1, mode='sum', keepdims=False, alpha=None):
    """The reduction ``mode`` of ``x`` over ``axis`` below ``seq_len`` (module docstring).  ``max`` returns ``(values, indices)``."""
    if mode not in MODES:
        raise ValueError(f'seq_pool: mode one of {sorted(MODES)}, got {mode!r}')
    alpha_t = alpha if torch.is_tensor(alpha) else None
    if x.dim() < 2 or x.numel() == 0:
        raise ValueError(f'seq_pool: x [B, ..., T, ...] with at least two axes, got {tuple(x.shape)}')
    ax = axis + x.dim() if axis < 0 else axis
    if not 1 <= ax < x.dim():
        raise ValueError(f'seq_pool: axis >= 1 (axis 0 is the batch), got {axis} for {x.dim()} axes')
    alpha0 = 0.
    if mode == 'autopool':
        if alpha is None:
            raise ValueError('seq_pool: autopool needs alpha')
        if alpha_t is not None:
            if x.dim() != 3 or ax != 2 or alpha_t.numel() != x.shape[1]:
                raise ValueError(f'seq_pool: a tensor alpha [C, 1] goes with x [B, C, T] and axis -1, got alpha {tuple(alpha_t.shape)}, '
                                 f'x {tuple(x.shape)}, axis {axis}')
        else:
            alpha0 = float(alpha)
    _check('seq_pool', x, alpha_t)
    lengths = device_lengths(seq_len, x.shape[0], x.device)
    y, index = _PoolFn.apply(x, lengths, alpha_t if mode == 'autopool' else None, alpha0, ax, MODES[mode])
    if keepdims:
        y = y.unsqueeze(ax)
        index = None if index is None else index.unsqueeze(ax)
    return (y, index) if mode == 'max' else y
