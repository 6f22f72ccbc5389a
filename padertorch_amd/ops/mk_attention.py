"""The kernels behind ``padertorch/contrib/mk/modules/transformer.py`` (``csrc/mk_attention.hip`` and the ``BIAS`` variant of
``csrc/attention.hip``).  fp32 on the GPU only; there is no CPU and no library fallback.

    qk_prepare(q, k, rms_q, rms_k, theta, l2, eps)    per-head RMS norm, rotary rotation and L2 normalisation of the projected queries
                                                      and keys ``[B, T, H, dh]`` in ONE launch (:681-689, :754-756)
    bias_attention(q, k, v, lengths, key_bias, slopes, causal)
                                                      ``softmax(q k^T / sqrt(d) + key_bias[b, j] - slopes[h] |j - i|) v`` without ever
                                                      writing a ``[B, H, Tq, Tk]`` tensor (:691-724)
    row_norm(kind, x, res, weight, bias, alpha, eps)  ``'layer'`` / ``'rms'`` / ``'dyt'`` norm of ``x (+ res)`` over the last axis; with ``res``
                                                      the sum is returned too, one launch for the add and the norm (:1002-1023)
    linear_slopes(H, device)                          ``linspace(8 / H, 8, H)``, made once per ``(H, device)`` on the host (:716-721)
"""
import math

import torch
from torch.autograd.function import once_differentiable

from .. import _lib
from . import attention as _attn
from . import library  # noqa: F401  (registers torch.ops.ptmi.attn_bias_*, mk_*)

__all__ = ['qk_prepare', 'bias_attention', 'row_norm', 'linear_slopes', 'KINDS', 'RMS_EPS']

#: ``row_norm``'s kinds, as ``ptmi_mk_row_norm_forward`` numbers them
KINDS = {'layer': 0, 'rms': 1, 'dyt': 2}
#: what ``nn.RMSNorm(eps=None)`` adds under the root for fp32 input
RMS_EPS = float(torch.finfo(torch.float32).eps)

_SLOPES = {}


def linear_slopes(H, device):
    """``torch.linspace(8 / H, 8, H)`` as the reference forms it on the host (:716-721), kept per ``(H, device)``: the kernel's slopes are
    the reference's bit for bit.  (The first call for an ``H`` copies 4 H bytes to the device: warm up before capturing a graph.)"""
    key = (int(H), *_lib.device_key(device))
    if key not in _SLOPES:
        _SLOPES[key] = torch.linspace(8 / H, 8, H).to(torch.float32).to(device)
    return _SLOPES[key]


def _check(name, *tensors):
    _lib.require_gpu(*tensors)
    for t in tensors:
        if t is not None and t.dtype != torch.float32:
            raise NotImplementedError(f'{name}: float32 only, got {t.dtype}')


def _flat(p):
    return None if p is None else p.detach().reshape(-1).contiguous()


class _QkPrepFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q, k, wq, wk, theta, l2, eps):
        qo, ko, q_irms, k_irms, q_il2, k_il2 = torch.ops.ptmi.mk_qk_prep_forward(q, k, _flat(wq), _flat(wk), theta, l2, eps)
        ctx.save_for_backward(q, k, wq, wk, theta, q_irms, k_irms, q_il2, k_il2)
        return qo, ko

    @staticmethod
    @once_differentiable
    def backward(ctx, gq, gk):
        q, k, wq, wk, theta, q_irms, k_irms, q_il2, k_il2 = ctx.saved_tensors
        dq, dk, dwq, dwk = torch.ops.ptmi.mk_qk_prep_backward(gq.contiguous(), None if k is None else gk.contiguous(), q, k, _flat(wq), _flat(wk),
                                                              theta, q_irms, k_irms, q_il2, k_il2)
        return dq, dk, (None if wq is None else dwq.view_as(wq)), (None if wk is None else dwk.view_as(wk)), None, None, None


def qk_prepare(q, k=None, rms_q=None, rms_k=None, theta=None, l2=False, eps=None):
    """``q [B, Tq, H, dh]`` and ``k [B, Tk, H, dh]`` (the projections' output as it lies; ``k=None``: ``q`` alone) through, in the
    reference's order and each optional: ``nn.RMSNorm(dh)`` with the weights ``rms_q`` / ``rms_k`` (``eps=None``: the fp32 epsilon),
    the rotary rotation of the pairs ``(2i, 2i+1)`` by ``(t + 1) theta[2i]`` (``theta``: ``RoPE``'s buffer, ``dh`` values) and
    ``F.normalize`` over ``dh`` (``l2``).  One launch forward, one backward; returns ``(q', k')`` in the operands' layout."""
    _check('qk_prepare', q, k, rms_q, rms_k, theta)
    if q.dim() != 4 or (k is not None and (k.dim() != 4 or k.shape[0] != q.shape[0] or k.shape[2:] != q.shape[2:])) or q.numel() == 0:
        raise ValueError(f'qk_prepare: q [B, Tq, H, dh], k [B, Tk, H, dh], got {tuple(q.shape)}, {None if k is None else tuple(k.shape)}')
    dh = q.shape[3]
    if dh % 2:
        raise NotImplementedError(f'qk_prepare: an odd head size ({dh}) has no rotary pairs')
    if dh > _attn.MAX_HEAD:
        raise NotImplementedError(f'qk_prepare: head sizes up to {_attn.MAX_HEAD}, got {dh}')
    if k is not None and (rms_q is None) != (rms_k is None):
        raise ValueError('qk_prepare: the RMS weights of q and k come together')
    theta = None if theta is None else theta.detach().reshape(-1).contiguous()
    return _QkPrepFn.apply(q.contiguous(), None if k is None else k.contiguous(), rms_q, rms_k, theta, bool(l2),
                           RMS_EPS if eps is None else float(eps))


class _BiasAttentionFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, q, k, v, lengths, causal, key_bias, slopes, scale):
        out, lse = torch.ops.ptmi.attn_bias_forward(q, k, v, lengths, causal, key_bias, slopes, scale)
        ctx.save_for_backward(q, k, v, lse, lengths, key_bias, slopes)       # (not out: the backward does not read it)
        ctx.cfg = (causal, scale)
        return out

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        q, k, v, lse, lengths, key_bias, slopes = ctx.saved_tensors
        causal, scale = ctx.cfg
        dq, dk, dv = torch.ops.ptmi.attn_bias_backward(q, k, v, _attn._unit_inner(g), lse, lengths, causal, key_bias, slopes, scale)
        need = ctx.needs_input_grad
        return (dq if need[0] else None), (dk if need[1] else None), (dv if need[2] else None), None, None, None, None, None


def bias_attention(q, k, v, lengths=None, key_bias=None, slopes=None, causal=False):
    """``ops.attention.attention`` with the additive score terms of mk's ``MultiheadAttention``: ``key_bias [B, Tk]`` (a float log-mask;
    ``-inf`` hides the key like a masked one) and ``slopes [H]`` (``- slopes[h] |j - i|``), neither with a gradient.  ``q, k, v`` are
    ``[B, H, T, d]`` views with a unit stride on ``d``; ``lengths`` (device int vector) still lets the kernel skip padded key tiles.
    Returns ``out [B, H, Tq, dv]``, a view of a contiguous ``[B, Tq, H, dv]``; no weights on this path."""
    q, k, v, _ = _attn._prepare('bias_attention', q, k, v, lengths, None)
    _check('bias_attention', key_bias, slopes)
    B, H, Tk = q.shape[0], q.shape[1], k.shape[2]
    if key_bias is not None and tuple(key_bias.shape) != (B, Tk):
        raise ValueError(f'bias_attention: key_bias [{B}, {Tk}], got {tuple(key_bias.shape)}')
    if slopes is not None and tuple(slopes.shape) != (H,):
        raise ValueError(f'bias_attention: one slope per head, [{H}], got {tuple(slopes.shape)}')
    key_bias = None if key_bias is None else _attn._unit_inner(key_bias.detach())
    slopes = None if slopes is None else slopes.detach().contiguous()
    return _BiasAttentionFn.apply(q, k, v, lengths, bool(causal), key_bias, slopes, 1. / math.sqrt(k.shape[3]))


class _RowNormFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, kind, a, res, weight, bias, alpha, eps):
        s, y, stats = torch.ops.ptmi.mk_row_norm_forward(kind, a, res, _flat(weight), _flat(bias), _flat(alpha), eps)
        ctx.save_for_backward(a if s is None else s, stats, weight, bias, alpha)
        ctx.kind = kind
        ctx.set_materialize_grads(False)
        return y if res is None else (s, y)

    @staticmethod
    @once_differentiable
    def backward(ctx, *grads):
        s, stats, weight, bias, alpha = ctx.saved_tensors
        gs, gy = (None, grads[0]) if len(grads) == 1 else grads
        if gy is None:
            gy = torch.zeros_like(s)
        need = ctx.needs_input_grad
        ds, dparams, dalpha = torch.ops.ptmi.mk_row_norm_backward(ctx.kind, gy.contiguous(), None if gs is None else gs.contiguous(), s, stats,
                                                                  _flat(weight), _flat(alpha), bool(need[3] or need[4]))
        N = s.shape[-1]
        return (None, ds, (ds if need[2] else None), (dparams[:N].view_as(weight) if need[3] else None),
                (dparams[N:].view_as(bias) if need[4] else None), (dalpha.view_as(alpha) if need[5] else None), None)


def row_norm(kind, x, res=None, weight=None, bias=None, alpha=None, eps=None):
    """The norm ``kind`` over the last axis of ``x`` - or of ``s = x + res``, and then ``(s, y)`` is returned: the residual add and the norm
    that follows it in one launch.  ``'layer'``: ``nn.LayerNorm`` (``eps`` 1e-5 by default), ``'rms'``: ``nn.RMSNorm`` (the fp32 epsilon by
    default, no bias), ``'dyt'``: ``tanh(alpha s) weight + bias`` with the one-element ``alpha`` read on the device.  ``weight`` / ``bias``
    may be absent.  Backward: one launch for the input gradient (the gradient arriving at ``s`` joins it there), weight and bias
    gradients and ``d alpha`` as ordered fp64 sums."""
    if kind not in KINDS:
        raise ValueError(f'row_norm: kind is one of {sorted(KINDS)}, got {kind!r}')
    _check('row_norm', x, res, weight, bias, alpha)
    N = x.shape[-1]
    if x.numel() == 0 or (res is not None and res.shape != x.shape) or any(p is not None and p.numel() != N for p in (weight, bias)) \
            or (kind == 'dyt') != (alpha is not None) or (kind == 'rms' and bias is not None):
        raise ValueError(f'row_norm({kind!r}): x, res [..., N], weight, bias [N], alpha [1] for dyt only; got {tuple(x.shape)}, '
                         f'{None if res is None else tuple(res.shape)}')
    if eps is None:
        eps = 1e-5 if kind == 'layer' else RMS_EPS
    return _RowNormFn.apply(KINDS[kind], x.contiguous(), None if res is None else res.contiguous(), weight, bias, alpha, float(eps))
