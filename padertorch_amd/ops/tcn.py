"""The non-GEMM part of a Conv-TasNet block on the HIP kernels of ``csrc/tcn.hip`` (``padertorch/modules/convnet.py:114-161``,
``padertorch/contrib/jensheit/norm.py:10-70``).  Activations are ``[B, T, C]`` with CHANNELS INNERMOST.

    depthwise_prelu(u, slope_in, weight, bias, slope_out, dilation, kernel_size)
        v = prelu(conv1d(pad(prelu(u)), weight, bias, groups=H, dilation)), padded 'both' to the input's length, and the per-example
        (mean, rstd) of v: returns (v [B, T, H], stats [B, 2])
    channel_norm(x, gamma, beta, groups='example' | 'row', stats=None, eps=1e-5)
        gamma (x - mean_g) rstd_g + beta: gLN (a group is an example) or cLN (a group is a row)
    pointwise_conv(x, weight, bias, residual=None)
        a 1x1 convolution: the split-fp16 GEMM of ops.gemm on the [B T, C] rows, the residual added by the GEMM's epilogue

All are differentiable in every floating input; forward and backward are kernels ("Conv-TasNet separator").  fp32 on the GPU
only: other dtypes raise ``NotImplementedError``, CPU tensors the "no CPU fallback" error.
"""
import torch
from torch.autograd.function import once_differentiable

from .. import _lib
from . import gemm as _gemm
from . import library  # noqa: F401  (registers torch.ops.ptmi.*)

__all__ = ['depthwise_prelu', 'channel_norm', 'pointwise_conv', 'depthwise_pad']


def depthwise_pad(kernel_size, dilation):
    """``(front, end)`` zero rows around the sequence: the reference's ``compute_pad_size(kernel_size, dilation, 1, 'both')`` - the window
    spans ``ks = 1 + dilation (kernel_size - 1)`` rows, ``front = (ks - 1) // 2``, ``end = ceil((ks - 1) / 2)``: an even kernel pads the
    end more."""
    span = dilation * (kernel_size - 1)
    return span // 2, span - span // 2


def _check(name, *tensors):
    _lib.require_gpu(*tensors)
    for t in tensors:
        if t is not None and t.dtype != torch.float32:
            raise NotImplementedError(f'{name}: float32 only, got {t.dtype}')


class _DepthwiseFn(torch.autograd.Function):
    """Kernels: ``tcn_depthwise_forward``; ``tcn_depthwise_backward`` (saves ``u`` alone: the pre-activation is recomputed)."""

    @staticmethod
    def forward(ctx, u, slope_in, weight, bias, slope_out, dilation, eps):
        u, weight = u.contiguous(), weight.contiguous()
        v, stats = torch.ops.ptmi.tcn_depthwise_forward(u, slope_in, weight, bias, slope_out, dilation, eps)
        ctx.save_for_backward(u, slope_in, weight, bias, slope_out)
        ctx.dilation = dilation
        ctx.mark_non_differentiable(stats)          # statistics OF v: channel_norm(v, stats=stats) differentiates through them
        return v, stats

    @staticmethod
    @once_differentiable
    def backward(ctx, gv, _gstats):
        u, slope_in, weight, bias, slope_out = ctx.saved_tensors
        gu, flat = torch.ops.ptmi.tcn_depthwise_backward(gv.contiguous(), u, slope_in, weight, bias, slope_out, ctx.dilation)
        n, h = weight.numel(), weight.shape[0]
        need = ctx.needs_input_grad
        return (gu if need[0] else None, flat[n + h:n + h + 1].view(slope_in.shape) if need[1] else None,
                flat[:n].view(weight.shape) if need[2] else None, flat[n:n + h] if bias is not None and need[3] else None,
                flat[n + h + 1:].view(slope_out.shape) if need[4] else None, None, None)


class _NormFn(torch.autograd.Function):
    """Kernels: ``tcn_norm_stats`` (unless the statistics are handed in), ``tcn_norm_apply``; ``tcn_norm_backward``."""

    @staticmethod
    def forward(ctx, x, gamma, beta, stats, rows, eps):
        x = x.contiguous()
        if stats is None:
            stats = torch.ops.ptmi.tcn_norm_stats(x, rows, eps)
        g, b = gamma.reshape(-1).contiguous(), beta.reshape(-1).contiguous()
        ctx.save_for_backward(x, g, stats)
        ctx.rows, ctx.shapes = rows, (gamma.shape, beta.shape)
        return torch.ops.ptmi.tcn_norm_apply(x, stats, g, b, rows)

    @staticmethod
    @once_differentiable
    def backward(ctx, gy):
        x, g, stats = ctx.saved_tensors
        dx, flat = torch.ops.ptmi.tcn_norm_backward(gy.contiguous(), x, stats, g, ctx.rows)
        c = g.numel()
        need = ctx.needs_input_grad
        return (dx if need[0] else None, flat[:c].view(ctx.shapes[0]) if need[1] else None,
                flat[c:].view(ctx.shapes[1]) if need[2] else None, None, None, None)


class _PointwiseFn(torch.autograd.Function):
    """``y = x W^T + bias (+ residual)`` on rows ``[M, C]``: three calls of ``ops.gemm.mm`` (forward, input gradient, weight gradient)."""

    @staticmethod
    def forward(ctx, x, weight, bias, residual):
        w = weight.reshape(weight.shape[0], -1)
        ctx.save_for_backward(x, weight)
        ctx.has_bias, ctx.has_residual = bias is not None, residual is not None
        if residual is None:
            return _gemm.mm(x, w.t(), bias=bias)
        return _gemm.mm(x, w.t(), bias=bias, out=residual.clone(memory_format=torch.contiguous_format), accumulate=True)

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        x, weight = ctx.saved_tensors
        w = weight.reshape(weight.shape[0], -1)
        g = g.contiguous()
        need = ctx.needs_input_grad
        dx = _gemm.mm(g, w) if need[0] else None
        dw = _gemm.mm(g.t(), x).view(weight.shape) if need[1] else None
        db = g.sum(0) if ctx.has_bias and need[2] else None
        return dx, dw, db, (g if ctx.has_residual and need[3] else None)


def depthwise_prelu(u, slope_in, weight, bias, slope_out, dilation, kernel_size, eps=1e-5):
    """``u [B, T, H]`` -> ``(v [B, T, H], stats [B, 2])``: ``v = prelu(slope_out, bias + sum_k weight[h, 0, k] p[t + k dilation - front])``
    with ``p = prelu(slope_in, u)``, zero outside ``[0, T)`` (:func:`depthwise_pad`: the reference pads behind the first PReLU), and
    ``stats[b] = (mean, 1 / sqrt(var + eps))`` of ``v[b]`` - what :func:`channel_norm` takes as ``stats`` for a gLN behind it.  ``weight
    [H, 1, K]``, ``bias [H]`` or None, slopes of one element each (``torch.nn.PReLU()``)."""
    _check('depthwise_prelu', u, slope_in, weight, bias, slope_out)
    if u.dim() != 3 or weight.dim() != 3 or tuple(weight.shape) != (u.shape[2], 1, kernel_size) or kernel_size < 1 or dilation < 1:
        raise ValueError(f'depthwise_prelu: u [B, T, H] and weight [H, 1, {kernel_size}], got {tuple(u.shape)}, {tuple(weight.shape)}')
    if slope_in.numel() != 1 or slope_out.numel() != 1 or (bias is not None and tuple(bias.shape) != (u.shape[2],)):
        raise ValueError('depthwise_prelu: one slope per PReLU and bias [H]')
    if u.numel() == 0:
        raise ValueError(f'depthwise_prelu: empty input {tuple(u.shape)}')
    return _DepthwiseFn.apply(u, slope_in, weight, bias, slope_out, int(dilation), float(eps))


def channel_norm(x, gamma, beta, groups='example', stats=None, eps=1e-5):
    """``gamma[c] (x - mean_g) / sqrt(var_g + eps) + beta[c]`` for ``x [B, T, C]`` (biased variance).  ``groups='example'``: statistics
    over ``T C`` (gLN); ``'row'``: over ``C`` (cLN).  ``gamma`` / ``beta`` hold ``C`` elements in any shape (``(C, 1)`` or ``(C,)``).
    ``stats [G, 2]``: ``(mean, rstd)`` OF THIS ``x`` computed elsewhere (:func:`depthwise_prelu`); the statistics pass is skipped and the
    gradient still flows through them as functions of ``x``."""
    _check('channel_norm', x, gamma, beta, stats)
    if groups not in ('example', 'row'):
        raise ValueError(f"channel_norm: groups 'example' or 'row', got {groups!r}")
    if x.dim() != 3 or gamma.numel() != x.shape[2] or beta.numel() != x.shape[2] or x.numel() == 0:
        raise ValueError(f'channel_norm: x [B, T, C] with C parameters each, got {tuple(x.shape)}, {tuple(gamma.shape)}, {tuple(beta.shape)}')
    rows = groups == 'row'
    if stats is not None:
        want = (x.shape[0] * x.shape[1] if rows else x.shape[0], 2)
        if tuple(stats.shape) != want:
            raise ValueError(f'channel_norm: stats {want}, got {tuple(stats.shape)}')
        stats = stats.detach().contiguous()
    return _NormFn.apply(x, gamma, beta, stats, rows, float(eps))


def pointwise_conv(x, weight, bias, residual=None):
    """``conv1d`` with a kernel of one on channel-last data: ``x [B, T, C]``, ``weight [H, C, 1]`` -> ``[B, T, H]`` (+ ``residual``)."""
    _check('pointwise_conv', x, weight, bias, residual)
    if x.dim() != 3 or weight.dim() != 3 or weight.shape[1] != x.shape[2] or weight.shape[2] != 1:
        raise ValueError(f'pointwise_conv: x [B, T, C] and weight [H, C, 1], got {tuple(x.shape)}, {tuple(weight.shape)}')
    B, T, C = x.shape
    res = None if residual is None else residual.reshape(B * T, weight.shape[0])
    return _PointwiseFn.apply(x.reshape(B * T, C), weight, bias, res).view(B, T, weight.shape[0])
