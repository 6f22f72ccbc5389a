"""The glue of the TasNet model on the HIP kernels of ``csrc/tasnet.hip``
(``padertorch/contrib/examples/source_separation/tasnet/model.py:86-142``): everything in ``TasNet.forward`` that is neither a coder, the
separator nor a 1x1 convolution.

    entry_norm(w, gamma, beta, lengths=None, eps=1e-5)
        ``w [B, N, E]`` (channels first, the encoder's output) -> ``[B, E, N]`` (channels last): the layer norm over the channels of every
        frame ``e < lengths[b]``, ZEROS on the frames behind (``apply_examplewise`` with its ``zeros_like`` buffer)
    prelu_rows(x, slope)
        ``x > 0 ? x : slope x`` with the one slope of ``torch.nn.PReLU()``
    mask_head(z, num_speakers, feature_size, additional_out_size=0, activation='sigmoid')
        ``z [B, E, A + K N]`` -> ``(m [K, B, N, E], additional [B, A, E] or None)``: slice, chunk, stack, transpose and nonlinearity
    center(d, samples)
        ``d [K, B, T']`` -> ``[B, K, min(samples, T')]``, cropped, the mean over the cropped length taken off

All are differentiable in every floating input; forward and backward are kernels ("TasNet model glue").  fp32 on the GPU
only: other dtypes raise ``NotImplementedError``, CPU tensors the "no CPU fallback" error.
"""
import torch
from torch.autograd.function import once_differentiable

from .. import _lib
from . import library  # noqa: F401  (registers torch.ops.ptmi.*)
from .library import TASNET_ACTIVATIONS

__all__ = ['entry_norm', 'prelu_rows', 'mask_head', 'center', 'TASNET_ACTIVATIONS']


def _check(name, *tensors):
    for t in tensors:                   # (the dtype first: a float64 tensor is refused for what it is, wherever it lives)
        if t is not None and t.dtype != torch.float32:
            raise NotImplementedError(f'{name}: float32 only, got {t.dtype}')
    _lib.require_gpu(*tensors)


class _EntryNormFn(torch.autograd.Function):
    """Kernels: ``tasnet_entry_norm_forward``; ``tasnet_entry_norm_backward`` (saves ``w`` and the row statistics, not ``y``)."""

    @staticmethod
    def forward(ctx, w, gamma, beta, lengths, eps):
        w, g, b = w.contiguous(), gamma.reshape(-1).contiguous(), beta.reshape(-1).contiguous()
        y, stats = torch.ops.ptmi.tasnet_entry_norm_forward(w, g, b, lengths, eps)
        ctx.save_for_backward(w, g, stats, lengths)
        ctx.shapes = (gamma.shape, beta.shape)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, gy):
        w, g, stats, lengths = ctx.saved_tensors
        dw, flat = torch.ops.ptmi.tasnet_entry_norm_backward(gy.contiguous(), w, stats, g, lengths)
        n = g.numel()
        need = ctx.needs_input_grad
        return (dw if need[0] else None, flat[:n].view(ctx.shapes[0]) if need[1] else None,
                flat[n:].view(ctx.shapes[1]) if need[2] else None, None, None)


class _PReLUFn(torch.autograd.Function):
    """Kernels: ``tasnet_prelu_forward``; ``tasnet_prelu_backward`` (saves the input)."""

    @staticmethod
    def forward(ctx, x, slope):
        x = x.contiguous()
        ctx.save_for_backward(x, slope)
        return torch.ops.ptmi.tasnet_prelu_forward(x, slope.contiguous())

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        x, slope = ctx.saved_tensors
        gx, da = torch.ops.ptmi.tasnet_prelu_backward(g.contiguous(), x, slope.contiguous())
        need = ctx.needs_input_grad
        return gx if need[0] else None, da.view(slope.shape) if need[1] else None


class _MaskHeadFn(torch.autograd.Function):
    """Kernels: ``tasnet_mask_head_forward``; ``tasnet_mask_head_backward`` (saves the output ``m``: ``z`` is not kept)."""

    @staticmethod
    def forward(ctx, z, K, N, A, activation):
        m, additional = torch.ops.ptmi.tasnet_mask_head_forward(z.contiguous(), K, N, A, activation)
        ctx.save_for_backward(m)
        ctx.A, ctx.activation = A, activation
        ctx.set_materialize_grads(False)
        return m, additional

    @staticmethod
    @once_differentiable
    def backward(ctx, gm, gadd):
        m, = ctx.saved_tensors
        if not ctx.needs_input_grad[0] or (gm is None and gadd is None):
            return None, None, None, None, None
        gm = torch.zeros_like(m) if gm is None else gm.contiguous()
        gadd = None if gadd is None or ctx.A == 0 else gadd.contiguous()
        return torch.ops.ptmi.tasnet_mask_head_backward(gm, m, gadd, ctx.A, ctx.activation), None, None, None, None


class _CenterFn(torch.autograd.Function):
    """Kernel pair ``tasnet_center`` forward, the same pair with the index maps exchanged backward (nothing is saved)."""

    @staticmethod
    def forward(ctx, d, samples):
        K, B, T_in = d.shape
        ctx.dims = (K, B, T_in, samples)
        return torch.ops.ptmi.tasnet_center(d.contiguous(), K, B, T_in, samples, False)

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        return torch.ops.ptmi.tasnet_center(g.contiguous(), *ctx.dims, True), None


def entry_norm(w, gamma, beta, lengths=None, eps=1e-5):
    """``w [B, N, E]`` -> ``y [B, E, N]``: ``y[b, e] = gamma (w[b, :, e] - mean) / sqrt(var + eps) + beta`` (statistics over the ``N``
    channels, biased variance: ``torch.nn.LayerNorm(N)``) for ``e < lengths[b]`` and ``0`` - not ``beta`` - for the frames behind.
    ``lengths``: ``[B]`` frames as an int32 / int64 tensor (on the GPU it is read by the kernel: a captured graph serves any pattern; a
    CPU tensor or a list is copied there), or None."""
    _check('entry_norm', w, gamma, beta)
    if w.dim() != 3 or gamma.numel() != w.shape[1] or beta.numel() != w.shape[1] or w.numel() == 0:
        raise ValueError(f'entry_norm: w [B, N, E] with N parameters each, got {tuple(w.shape)}, {tuple(gamma.shape)}, {tuple(beta.shape)}')
    if lengths is not None:
        if not torch.is_tensor(lengths):
            lengths = torch.tensor([int(n) for n in lengths], dtype=torch.int64)
        if lengths.dtype not in (torch.int32, torch.int64) or tuple(lengths.shape) != (w.shape[0],):
            raise ValueError(f'entry_norm: lengths [B] int32 or int64, got {lengths.dtype} {tuple(lengths.shape)}')
        lengths = lengths.to(w.device).contiguous()
    return _EntryNormFn.apply(w, gamma, beta, lengths, float(eps))


def prelu_rows(x, slope):
    """``x > 0 ? x : slope x`` for ``x`` of any shape and ONE slope (``torch.nn.PReLU().weight``); at ``x == 0`` the derivative is
    ``slope``, as in ``depthwise_prelu``."""
    _check('prelu_rows', x, slope)
    if slope.numel() != 1 or x.numel() == 0:
        raise ValueError(f'prelu_rows: one slope and a non-empty input, got {tuple(slope.shape)}, {tuple(x.shape)}')
    return _PReLUFn.apply(x, slope)


def mask_head(z, num_speakers, feature_size, additional_out_size=0, activation='sigmoid'):
    """``z [B, E, A + K N]`` (the output projection, channels last) -> ``(m [K, B, N, E], additional)`` with
    ``m[k, b, n, e] = act(z[b, e, A + k N + n])`` and ``additional [B, A, E] = z[b, e, :A]`` without activation (None when ``A == 0``):
    ``model.py:104-113`` and the transpose back to the coders' layout.  ``activation``: a key of ``TASNET_ACTIVATIONS``."""
    if activation not in TASNET_ACTIVATIONS:
        raise ValueError(f'mask_head: activation one of {sorted(TASNET_ACTIVATIONS)}, got {activation!r}')
    _check('mask_head', z)
    K, N, A = int(num_speakers), int(feature_size), int(additional_out_size)
    if z.dim() != 3 or K < 1 or N < 1 or A < 0 or z.shape[2] != A + K * N or z.numel() == 0:
        raise ValueError(f'mask_head: z [B, E, {A} + {K} * {N}], got {tuple(z.shape)}')
    m, additional = _MaskHeadFn.apply(z, K, N, A, TASNET_ACTIVATIONS[activation])
    return m, (additional if A else None)


def center(d, samples):
    """``d [K, B, T']`` -> ``out [B, K, T_out]``, ``T_out = min(samples, T')``: ``out[b, k] = d[k, b, :T_out] - mean(d[k, b, :T_out])``
    (``model.py:133-142``; the mean runs over the padded batch length, not over an example's own)."""
    _check('center', d)
    if d.dim() != 3 or d.numel() == 0 or int(samples) < 1:
        raise ValueError(f'center: d [K, B, T] and samples >= 1, got {tuple(d.shape)}, {samples}')
    return _CenterFn.apply(d, min(int(samples), d.shape[2]))

