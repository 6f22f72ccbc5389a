"""The TasNet learned-basis coders on the HIP kernels of ``csrc/tas_coders.hip``
(``padertorch/contrib/examples/source_separation/tasnet/tas_coders.py:9-135``, ``tasnet/model.py:119-129``).

    tas_encode(x, weight, bias, stride, window_length)        relu(conv1d(zero-padded x)): TasEncoder.forward
    tas_decode(w, weight, bias, stride)                       conv_transpose1d(w)[:, 0]:   TasDecoder.forward
    tas_masked_decode(mask, encoded, weight, bias, stride)    tas_decode(mask[k] * encoded) for every k, without the product in memory

Each is differentiable in every floating input; forward and backward are kernels of three families (analysis, synthesis, weight
gradient: DESIGN.md, "TasNet learned-basis coders").  fp32 on the GPU only: other dtypes raise ``NotImplementedError``, CPU tensors the
"no CPU fallback" error.
"""
import torch
from torch.autograd.function import once_differentiable

from .. import _lib
from . import library  # noqa: F401  (registers torch.ops.ptmi.*)

__all__ = ['tas_encode', 'tas_decode', 'tas_masked_decode', 'tas_encoded_frames', 'tas_encoded_lengths']


def _padded_samples(samples, window_length):
    """The signal length after the reference's zero padding to a multiple of HALF A WINDOW (not of the stride; ``tas_coders.py:73-76``)."""
    h = window_length // 2
    return samples if samples % h == 0 else samples + h - samples % h


def tas_encoded_frames(samples, window_length, stride):
    """Frames the encoder returns for ``samples`` input samples."""
    padded = _padded_samples(samples, window_length)
    if padded < window_length:
        raise RuntimeError(f'tas_encode: {samples} samples are shorter than one window of {window_length}')
    return (padded - window_length) // stride + 1


def tas_encoded_lengths(sequence_lengths, samples, window_length):
    """``sequence_lengths // (L // 2)``, minus one unless the batch was padded - whatever the stride is (``tas_coders.py:71-81``)."""
    if sequence_lengths is None:
        return None
    h = window_length // 2
    return sequence_lengths // h + (0 if samples % h > 0 else -1)


def _check(name, *tensors):
    _lib.require_gpu(*tensors)
    for t in tensors:
        if t is not None and t.dtype != torch.float32:
            raise NotImplementedError(f'{name}: float32 only, got {t.dtype}')


def _weight_grads(ctx, flat, weight, bias_at):
    """``flat`` (``tas_wgrad``) -> the gradients of ``weight`` and of the bias: the per-row sums of an encoder, the total of a decoder."""
    nl, n = weight.numel(), weight.shape[0]
    dw = flat[:nl].view(weight.shape) if ctx.needs_input_grad[ctx.weight_arg] else None
    db = None
    if ctx.has_bias and ctx.needs_input_grad[ctx.weight_arg + 1]:
        db = flat[nl:nl + n] if bias_at == 'rows' else flat[nl + n:]
    return dw, db


class _EncodeFn(torch.autograd.Function):
    """Kernels: ``tas_analysis`` forward; ``tas_synthesis`` (gated by the saved output) and ``tas_wgrad`` backward."""

    @staticmethod
    def forward(ctx, x, weight, bias, stride, frames):
        x, weight = x.contiguous(), weight.contiguous()
        bias = None if bias is None else bias.contiguous()
        w = torch.ops.ptmi.tas_analysis(x, weight, bias, stride, frames, True)
        ctx.save_for_backward(x, weight, w)
        ctx.has_bias, ctx.stride, ctx.weight_arg = bias is not None, stride, 1
        return w

    @staticmethod
    @once_differentiable
    def backward(ctx, gw):
        x, weight, w = ctx.saved_tensors
        gw = gw.contiguous()
        dx = dw = db = None
        if ctx.needs_input_grad[0]:
            dx = torch.ops.ptmi.tas_synthesis(gw, None, w, weight, None, ctx.stride, x.shape[1])
        if ctx.needs_input_grad[1] or (ctx.has_bias and ctx.needs_input_grad[2]):
            flat = torch.ops.ptmi.tas_wgrad(gw, None, w, x, ctx.stride, weight.shape[-1])
            dw, db = _weight_grads(ctx, flat, weight, 'rows')
        return dx, dw, db, None, None


class _DecodeFn(torch.autograd.Function):
    """Kernels: ``tas_synthesis`` forward; ``tas_analysis`` (identity) and ``tas_wgrad`` backward."""

    @staticmethod
    def forward(ctx, w, weight, bias, stride):
        w, weight = w.contiguous(), weight.contiguous()
        samples = (w.shape[2] - 1) * stride + weight.shape[-1]
        y = torch.ops.ptmi.tas_synthesis(w, None, None, weight, bias, stride, samples)
        ctx.save_for_backward(w, weight)
        ctx.has_bias, ctx.stride, ctx.weight_arg = bias is not None, stride, 1
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, gy):
        w, weight = ctx.saved_tensors
        gy = gy.contiguous()
        dw_in = dw = db = None
        if ctx.needs_input_grad[0]:
            dw_in = torch.ops.ptmi.tas_analysis(gy, weight, None, ctx.stride, w.shape[2], False)
        if ctx.needs_input_grad[1] or (ctx.has_bias and ctx.needs_input_grad[2]):
            flat = torch.ops.ptmi.tas_wgrad(w, None, None, gy, ctx.stride, weight.shape[-1])
            dw, db = _weight_grads(ctx, flat, weight, 'total')
        return dw_in, dw, db, None


class _MaskedDecodeFn(torch.autograd.Function):
    """Kernels: ``tas_synthesis`` (masked) forward; ``tas_masked_decode_backward`` and ``tas_wgrad`` (masked) backward."""

    @staticmethod
    def forward(ctx, mask, encoded, weight, bias, stride):
        mask, encoded, weight = mask.contiguous(), encoded.contiguous(), weight.contiguous()
        samples = (encoded.shape[2] - 1) * stride + weight.shape[-1]
        y = torch.ops.ptmi.tas_synthesis(encoded, mask, None, weight, bias, stride, samples)
        ctx.save_for_backward(mask, encoded, weight)
        ctx.has_bias, ctx.stride, ctx.weight_arg = bias is not None, stride, 2
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, gy):
        mask, encoded, weight = ctx.saved_tensors
        gy = gy.contiguous()
        dm = de = dw = db = None
        if ctx.needs_input_grad[0] or ctx.needs_input_grad[1]:
            dm, de = torch.ops.ptmi.tas_masked_decode_backward(gy, mask, encoded, weight, ctx.stride)
            dm = dm if ctx.needs_input_grad[0] else None
            de = de if ctx.needs_input_grad[1] else None
        if ctx.needs_input_grad[2] or (ctx.has_bias and ctx.needs_input_grad[3]):
            flat = torch.ops.ptmi.tas_wgrad(encoded, mask, None, gy, ctx.stride, weight.shape[-1])
            dw, db = _weight_grads(ctx, flat, weight, 'total')
        return dm, de, dw, db, None


def _coder_weight(name, weight, bias, bias_size):
    if weight.dim() != 3 or weight.shape[1] != 1:
        raise ValueError(f'{name}: weight [N, 1, L], got {tuple(weight.shape)}')
    if bias is not None and tuple(bias.shape) != (bias_size,):
        raise ValueError(f'{name}: bias [{bias_size}], got {tuple(bias.shape)}')


def tas_encode(x, weight, bias, stride, window_length):
    """``relu(conv1d(pad(x)[:, None], weight, bias, stride))`` for ``x [B, T]``: ``[B, N, frames]``.  ``x`` counts as zero-padded at the end
    to a multiple of ``window_length // 2`` (the kernels read the padding as zeros; nothing is copied)."""
    _check('tas_encode', x, weight, bias)
    _coder_weight('tas_encode', weight, bias, weight.shape[0])
    if x.dim() != 2 or weight.shape[2] != window_length or window_length < 2 or stride < 1:
        raise ValueError(f'tas_encode: x [B, T] and weight [N, 1, {window_length}], got {tuple(x.shape)}, {tuple(weight.shape)}')
    frames = tas_encoded_frames(x.shape[1], window_length, stride)
    return _EncodeFn.apply(x, weight, bias, int(stride), frames)


def tas_decode(w, weight, bias, stride):
    """``conv_transpose1d(w, weight, bias, stride)[:, 0]`` for ``w [B, N, frames]``: ``[B, (frames - 1) * stride + L]``."""
    _check('tas_decode', w, weight, bias)
    _coder_weight('tas_decode', weight, bias, 1)
    if w.dim() != 3 or w.shape[1] != weight.shape[0] or stride < 1:
        raise ValueError(f'tas_decode: w [B, {weight.shape[0]}, frames], got {tuple(w.shape)}')
    return _DecodeFn.apply(w, weight, bias, int(stride))


def tas_masked_decode(mask, encoded, weight, bias, stride):
    """``tas_decode(mask[k] * encoded)`` for every ``k``: ``mask [K, B, N, frames]``, ``encoded [B, N, frames]`` ->
    ``[K, B, (frames - 1) * stride + L]``.  The product never exists in memory, forward or backward."""
    _check('tas_masked_decode', mask, encoded, weight, bias)
    _coder_weight('tas_masked_decode', weight, bias, 1)
    if encoded.dim() != 3 or mask.dim() != 4 or tuple(mask.shape[1:]) != tuple(encoded.shape) or encoded.shape[1] != weight.shape[0] \
            or stride < 1:
        raise ValueError(f'tas_masked_decode: mask [K, B, N, frames] and encoded [B, N, frames] with N = {weight.shape[0]}, got '
                         f'{tuple(mask.shape)}, {tuple(encoded.shape)}')
    return _MaskedDecodeFn.apply(mask, encoded, weight, bias, int(stride))
