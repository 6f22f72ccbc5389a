"""Fused scaled-dot-product attention and the transformer layer's glue on ``csrc/attention.hip`` (reference:
``padertorch/contrib/je/modules/transformer.py``).  fp32 on the GPU only; there is no CPU and no library fallback.

    scaled_dot_product_attention(q, k, v, seq_len=None, bidirectional=False, mask=None, need_weights=True)
                                          the reference's function (:12-38): (out, weights), out differentiable in q, k, v
    attention(q, k, v, lengths, causal, mask)   the same on ``[B, H, T, d]`` views, out only: what MultiHeadAttention calls
    positional_encoding_(x)               x [B, T, d] += the interleaved cos / sin encoding, in place (:234-243); backward: the identity
    norm_residual(z, res, gamma, beta, lengths, eps, norm_first)
                                          masked LayerNorm over the channels + residual in one launch (:151-155 with norm='layer')

The ``[B, H, Tq, Tk]`` score tensor is never written unless the weights are asked for.  Two departures from the reference: the returned
``weights`` carry NO gradient (nothing in the reference differentiates through them), and the head sizes are limited to
``MAX_HEAD = 128`` (``NotImplementedError`` beyond).  A query row without a visible key is NaN in ``out`` and ``weights`` as in the
reference; it contributes nothing to the gradients (the reference's are NaN then).
"""
import math

import torch
from torch.autograd.function import once_differentiable

from .. import _lib
from . import library  # noqa: F401  (registers torch.ops.ptmi.attn_*, transformer_*)

__all__ = ['scaled_dot_product_attention', 'attention', 'positional_encoding_', 'norm_residual', 'device_lengths', 'MAX_HEAD', 'TILE',
           'KEY_TILE']

#: the largest head size of the kernels (``NotImplementedError`` beyond)
MAX_HEAD = 128
#: rows a workgroup owns / rows of a streamed tile (``ptmi_attn_tile`` / ``ptmi_attn_key_tile``): what the tests put Tq and Tk around
TILE, KEY_TILE = 64, 32


def _check(name, *tensors):
    _lib.require_gpu(*tensors)
    for t in tensors:
        if t is not None and t.dtype != torch.float32:
            raise NotImplementedError(f'{name}: float32 only, got {t.dtype}')


def device_lengths(seq_len, device):
    """``seq_len`` (None, host list / array, CPU or device tensor) as an int32 or int64 DEVICE vector without a host synchronisation."""
    if seq_len is None:
        return None
    if torch.is_tensor(seq_len) and seq_len.is_cuda:
        return (seq_len if seq_len.dtype in (torch.int32, torch.int64) else seq_len.long()).contiguous()
    return _lib.host_to_device(seq_len, torch.int32, device)


def _unit_inner(t):
    return t if t.stride(-1) == 1 or t.shape[-1] == 1 else t.contiguous()


class _AttentionFn(torch.autograd.Function):
    """``q, k, v [B, H, T, d]`` (any strides, unit on ``d``) -> ``out [B, H, Tq, dv]``; saves ``lse`` and recomputes the probabilities."""

    @staticmethod
    def forward(ctx, q, k, v, lengths, causal, mask, scale):
        out, lse = torch.ops.ptmi.attn_forward(q, k, v, lengths, causal, mask, scale)
        ctx.save_for_backward(q, k, v, out, lse, lengths, mask)
        ctx.cfg = (causal, scale)
        ctx.mark_non_differentiable(lse)
        return out, lse

    @staticmethod
    @once_differentiable
    def backward(ctx, g, _glse):
        q, k, v, out, lse, lengths, mask = ctx.saved_tensors
        causal, scale = ctx.cfg
        dq, dk, dv = torch.ops.ptmi.attn_backward(q, k, v, out, _unit_inner(g), lse, lengths, causal, mask, scale)
        need = ctx.needs_input_grad
        return (dq if need[0] else None), (dk if need[1] else None), (dv if need[2] else None), None, None, None, None


def _prepare(name, q, k, v, lengths, mask):
    _check(name, q, k, v)
    if not (q.dim() == k.dim() == v.dim() == 4) or q.shape[:2] != k.shape[:2] or k.shape[:3] != v.shape[:3] or q.shape[3] != k.shape[3] \
            or q.numel() == 0 or k.numel() == 0 or v.numel() == 0:
        raise ValueError(f'{name}: q [B, H, Tq, d], k [B, H, Tk, d], v [B, H, Tk, dv], got {tuple(q.shape)}, {tuple(k.shape)}, {tuple(v.shape)}')
    if q.shape[3] > MAX_HEAD or v.shape[3] > MAX_HEAD:
        raise NotImplementedError(f'{name}: head sizes up to {MAX_HEAD} (the limit of the fused kernels, which hold a head in registers); '
                                  f'got {q.shape[3]} and {v.shape[3]}')
    B, H, Tq, _ = q.shape
    Tk = k.shape[2]
    if lengths is not None and tuple(lengths.shape) != (B,):
        raise ValueError(f'{name}: one key count per example, [{B}], got {tuple(lengths.shape)}')
    if mask is not None:
        _lib.require_gpu(mask)
        if mask.dtype not in (torch.bool, torch.uint8):
            mask = mask > 0
        mask = mask.expand(B, H, Tq, Tk)                    # broadcast axes get stride 0: read through strides, never copied
    return _unit_inner(q), _unit_inner(k), _unit_inner(v), mask


def attention(q, k, v, lengths=None, causal=False, mask=None, need_weights=False):
    """``softmax(q k^T / sqrt(d) + masks) v`` for ``q [B, H, Tq, d]``, ``k [B, H, Tk, d]``, ``v [B, H, Tk, dv]`` given as ANY views with a unit
    stride on the last axis (the ``[B, T, H, d]`` projection output transposed, a ``transpose(1, 2)`` of anything, ...): no copies.
    ``lengths``: int32 / int64 device vector ``[B]`` of key counts; ``causal``: query ``i`` sees keys ``j <= i + Tk - Tq``; ``mask``:
    broadcastable to ``[B, H, Tq, Tk]``, ``> 0`` keeps.  All given masks apply.  Returns ``out [B, H, Tq, dv]``, a view of a contiguous
    ``[B, Tq, H, dv]`` (so ``out.transpose(1, 2).reshape(B, Tq, H dv)`` is free), and the weights ``[B, H, Tq, Tk]`` (no gradient) or, without
    ``need_weights``, ``None`` - the kernel that writes them is launched only when they are asked for."""
    q, k, v, mask = _prepare('attention', q, k, v, lengths, mask)
    scale = 1. / math.sqrt(k.shape[3])
    out, lse = _AttentionFn.apply(q, k, v, lengths, bool(causal), mask, scale)
    weights = None
    if need_weights:
        with torch.no_grad():
            weights = torch.ops.ptmi.attn_weights(q.detach(), k.detach(), lse, lengths, bool(causal), mask, scale)
    return out, weights


def _as4(t):
    """``[..., T, d]`` -> ``[B, H, T, d]`` (B the first axis: the one the lengths count; views where the shape allows)."""
    if t.dim() == 2:
        return t[None, None]
    if t.dim() == 3:
        return t[:, None]
    return t if t.dim() == 4 else t.reshape(t.shape[0], -1, *t.shape[-2:])


def scaled_dot_product_attention(q, k, v, seq_len=None, bidirectional=False, mask=None, need_weights=True):
    """The reference's function (transformer.py:12-38) for ``q [..., Tq, d]``, ``k [..., Tk, d]``, ``v [..., Tk, dv]``: returns ``(out
    [..., Tq, dv], weights [..., Tq, Tk])``.  The masks take the reference's precedence: with ``bidirectional=False`` the causal mask
    (diagonal ``Tk - Tq``) applies and ``seq_len`` is IGNORED (the ``elif`` at :31-36); with ``bidirectional=True`` and ``seq_len`` given
    the keys ``j >= seq_len[b]`` are masked (``b`` the first axis); ``mask`` (``> 0`` keeps) applies in both cases.

    ``out`` is differentiable in ``q``, ``k``, ``v``.  Departure from the reference: ``weights`` carry no gradient (nothing in the reference
    differentiates through them); ``need_weights=False`` returns ``None`` in their place and does not launch the kernel that writes them.
    Head sizes up to ``MAX_HEAD``."""
    _check('scaled_dot_product_attention', q, k, v)
    if q.dim() < 2 or q.dim() != k.dim() or k.dim() != v.dim() or q.shape[:-2] != k.shape[:-2] or k.shape[:-1] != v.shape[:-1]:
        raise ValueError(f'scaled_dot_product_attention: q [..., Tq, d], k [..., Tk, d], v [..., Tk, dv], got {tuple(q.shape)}, '
                         f'{tuple(k.shape)}, {tuple(v.shape)}')
    lead, Tq, Tk = q.shape[:-2], q.shape[-2], k.shape[-2]
    lengths = device_lengths(seq_len, q.device) if bidirectional else None
    if mask is not None:
        _lib.require_gpu(mask)
        if mask.dtype not in (torch.bool, torch.uint8):
            mask = mask > 0
        mask = _as4(mask.expand(*lead, Tq, Tk))
    out, weights = attention(_as4(q), _as4(k), _as4(v), lengths, not bidirectional, mask, need_weights)
    return out.reshape(*lead, Tq, v.shape[-1]), (weights.reshape(*lead, Tq, Tk) if need_weights else None)


# ------------------------------------------------------------------------------------------------ glue
class _PosEncFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, freq):
        torch.ops.ptmi.transformer_posenc_(x, freq)
        ctx.mark_dirty(x)
        return x

    @staticmethod
    def backward(ctx, g):
        return g, None


_FREQ = {}


def posenc_frequencies(d, device):
    """``10000^(2i/d)``, ``i < d / 2``, as the float32 tensor the reference's expression gives (transformer.py:239: an int64 ``arange``, a
    python float, torch's float32 ``pow`` on the host) - made once per ``(d, device)`` and kept, so the kernel's angles ``t / freq[i]``
    are the reference's bit for bit.  (The first call for a ``d`` copies 2 d bytes to the device: warm up before capturing a graph.)"""
    key = (int(d), *_lib.device_key(device))
    if key not in _FREQ:
        _FREQ[key] = (10000 ** (2 * torch.arange(d // 2) / d)).to(torch.float32).to(device)
    return _FREQ[key]


def positional_encoding_(x):
    """``x[b, t, 2i] += cos(t / 10000^(2i/d))``, ``x[b, t, 2i+1] += sin(same)`` IN PLACE on a contiguous ``x [B, T, d]``, ``d`` even
    (transformer.py:234-243); accurate ``cosf`` / ``sinf``, the angle taken in fp32 as the reference takes it."""
    _check('positional_encoding_', x)
    if x.dim() != 3 or x.shape[2] % 2 or not x.is_contiguous() or x.numel() == 0:
        raise ValueError(f'positional_encoding_: a contiguous [B, T, d] with d even, got {tuple(x.shape)} strides {x.stride()}')
    return _PosEncFn.apply(x, posenc_frequencies(x.shape[2], x.device))


class _NormResidualFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, z, res, gamma, beta, lengths, eps, norm_first):
        y, u, stats = torch.ops.ptmi.transformer_norm_residual_forward(z, res, gamma.detach().reshape(-1), beta.detach().reshape(-1), lengths,
                                                                       eps, norm_first)
        ctx.save_for_backward(z if norm_first else u, stats, gamma, lengths)
        ctx.norm_first = norm_first
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        v, stats, gamma, lengths = ctx.saved_tensors
        need = ctx.needs_input_grad
        N = v.shape[2]
        g = g.contiguous()
        dv, dparams = torch.ops.ptmi.transformer_norm_residual_backward(g, v, stats, gamma.detach().reshape(-1), lengths, need[2] or need[3])
        dres = g if ctx.norm_first else dv
        return ((dv if need[0] else None), (dres if need[1] else None), (dparams[:N].view_as(gamma) if need[2] else None),
                (dparams[N:].view_as(gamma) if need[3] else None), None, None, None)


def norm_residual(z, res, gamma, beta, lengths=None, eps=1e-2, norm_first=True):
    """``norm_first``: ``LN(z) + res``; else ``LN(z + res)``.  ``LN`` is the masked layer norm over the channels of ``[B, T, N]`` with ``gamma``,
    ``beta`` (``N`` values each, any shape) and zeros for ``t >= lengths[b]``, as ``Normalization(data_format='btc', statistics_axis='c')``
    gives it; one launch forward, the ``gamma`` / ``beta`` gradients as ordered fp64 column sums."""
    _check('norm_residual', z, res, gamma, beta)
    if z.dim() != 3 or z.shape != res.shape or gamma.numel() != z.shape[2] or beta.numel() != z.shape[2] or z.numel() == 0:
        raise ValueError(f'norm_residual: z, res [B, T, N], gamma, beta [N], got {tuple(z.shape)}, {tuple(res.shape)}, {tuple(gamma.shape)}, '
                         f'{tuple(beta.shape)}')
    return _NormResidualFn.apply(z.contiguous(), res.contiguous(), gamma, beta, lengths, float(eps), bool(norm_first))
