"""The contrast of contrastive predictive coding (``padertorch/contrib/mk/modules/contrastive.py:343-471``, ``CPC1d.contrast``) fused
with the cross-entropy, ``argmax`` and ``> -inf`` count of its ``review`` (``:515-540``) on the kernels of ``csrc/cpc_contrast.hip``
(DESIGN.md 3.5t).

    contrastive_scores(z_hat [b, S d, t], z [b, d, t], steps, mode, temperature=1., negative_to_target_dist=0,
                       log_batch_mask=None, negative_ratio=1., dense=False)
        -> [ContrastStats(ce, hits, finite, logits) per step]        each [b, T_s], T_s = t - |step|; logits [b, K, T_s] or None

Step ``s`` contrasts query ``z_hat[:, s d:(s + 1) d, q + max(-s, 0)]`` with

    'time'   the ``K = t`` keys ``z[i, :, (k + max(s, 0)) mod t]`` of its own batch entry (the reference's ``torch.roll``: wrapped keys and
             frames behind a sequence's length ARE keys); target ``k = q``
    'all'    the ``K = b t`` keys of every entry, flat index ``i' t + k``; target ``i t + q``
    'batch'  the ``K = b`` keys ``z[:, :, q + max(s, 0)]``; target ``i``; ``log_batch_mask [b, b]`` is added and, with ``negative_ratio < 1``,
             key ``j`` stays iff ``score_j <= (the kk-th largest of the row)`` or ``j`` is the target, ``kk = max(ceil(b (1 - ratio)), 1)``

``score = <query, key> / temperature``; in 'time' / 'all' the keys of the query's own entry with ``0 < |k - q| <= dist - 1`` are ``-inf``.
``ce = logsumexp - target score`` (differentiable with respect to ``z_hat`` and ``z``), ``hits`` = 1 where the first maximal key is the
target, ``finite`` = number of keys with a score ``> -inf`` (int32).  The default path allocates nothing of size ``K``: the forward is
one launch that keeps an online log-sum-exp per query, the backward two launches ('time' / 'all': a query-owning kernel for ``dz_hat`` and
a frame-owning kernel for ``dz``) or one ('batch') that recompute the scores from the saved log-sum-exp.  No host reads, no atomics:
forward + backward capture into a graph.  ``dense=True`` also stores the reference's logits from the forward's tile epilogue.

fp32 on the GPU only; ``d <= max_features()`` (512), at most 16 steps, ``b <= max_batch()`` (64) for 'batch'; ``NotImplementedError``
beyond.  Dot-product similarity only.
"""
import math
from collections import namedtuple

import torch
from torch.autograd.function import once_differentiable

from .. import _lib
from . import library  # noqa: F401  (registers torch.ops.ptmi.cpc_*)

__all__ = ['contrastive_scores', 'ContrastStats', 'MODES', 'max_features', 'max_batch', 'kCpcBM', 'kCpcBN']

MODES = {'time': 0, 'all': 1, 'batch': 2}
ContrastStats = namedtuple('ContrastStats', ['ce', 'hits', 'finite', 'logits'])

#: queries a workgroup owns / key indices of a streamed tile (``ptmi_cpc_query_tile()`` / ``ptmi_cpc_key_tile()``): what the tests put t around
kCpcBM, kCpcBN = 64, 32


def max_features():
    """``ptmi_cpc_max_features()``: the largest feature size the kernels stage (a host function of the library: no GPU needed)."""
    return int(_lib.load().ptmi_cpc_max_features())


def max_batch():
    """``ptmi_cpc_max_batch()``: the largest batch of ``mode='batch'`` (the whole ``b x b`` row block sits in LDS)."""
    return int(_lib.load().ptmi_cpc_max_batch())


class _ContrastFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, z_hat, z, log_batch_mask, steps, mode, temperature, dist, keep, dense):
        stats, logits = torch.ops.ptmi.cpc_forward(z_hat, z, steps, mode, temperature, dist, log_batch_mask, keep, dense)
        ctx.save_for_backward(z_hat, z, log_batch_mask, stats)
        ctx.cfg = (steps, mode, temperature, dist, keep)
        ce, hits, finite = stats[0], stats[1], stats[2].view(torch.int32)
        ctx.mark_non_differentiable(hits, finite)
        if logits is None:
            return ce, hits, finite
        ctx.mark_non_differentiable(logits)
        return ce, hits, finite, logits

    @staticmethod
    @once_differentiable
    def backward(ctx, g, *_):
        z_hat, z, log_batch_mask, stats = ctx.saved_tensors
        dz_hat, dz = torch.ops.ptmi.cpc_backward(z_hat, z, *ctx.cfg[:4], log_batch_mask, ctx.cfg[4], stats[3], g.contiguous())
        return dz_hat, dz, None, None, None, None, None, None, None


def contrastive_scores(z_hat, z, steps, mode, temperature=1., negative_to_target_dist=0, log_batch_mask=None, negative_ratio=1.,
                       dense=False):
    """The per-step statistics of the module docstring, one :class:`ContrastStats` per entry of ``steps``."""
    if mode not in MODES:
        raise ValueError(f'Unknown negatives_mode {mode}')
    steps = [int(s) for s in steps]
    if z.dim() != 3 or z_hat.dim() != 3 or not steps or z_hat.shape != (z.shape[0], len(steps) * z.shape[1], z.shape[2]):
        raise ValueError(f'contrastive_scores: z [b, d, t] and z_hat [b, {len(steps)} d, t], got {tuple(z.shape)}, {tuple(z_hat.shape)}')
    b, d, t = z.shape
    if max(abs(s) for s in steps) >= t:
        raise ValueError(f'contrastive_scores: steps {steps} leave no frame of t = {t}')
    for x in (z, z_hat, log_batch_mask):
        if x is not None and x.dtype != torch.float32:
            raise NotImplementedError(f'contrastive_scores: float32 only, got {x.dtype}')
    _lib.require_gpu(z, z_hat, log_batch_mask)
    if d > max_features():
        raise NotImplementedError(f'contrastive_scores: {d} features; the kernels stage up to {max_features()} (ptmi_cpc_max_features)')
    if mode == 'batch' and b > max_batch():
        raise NotImplementedError(f'contrastive_scores: negatives_mode="batch" with b = {b}; the row block in LDS takes up to {max_batch()} '
                                  f'(ptmi_cpc_max_batch)')
    if z.stride(2) != 1:
        z = z.contiguous()
    if z_hat.stride(2) != 1:
        z_hat = z_hat.contiguous()
    keep = 1
    if mode == 'batch':
        keep = max(int(math.ceil(b * (1 - negative_ratio))), 1)
        if log_batch_mask is not None:
            log_batch_mask = log_batch_mask.reshape(b, b).contiguous()
    else:
        log_batch_mask = None
    out = _ContrastFn.apply(z_hat, z, log_batch_mask, steps, MODES[mode], float(temperature), int(negative_to_target_dist), keep,
                            bool(dense))
    K = {'time': t, 'all': b * t, 'batch': b}[mode]
    stats, row, el = [], 0, 0
    for s in steps:
        Ts = t - abs(s)
        ce, hits, finite = (x[row:row + b * Ts].view(b, Ts) for x in (out[0], out[1].detach(), out[2].detach()))
        stats.append(ContrastStats(ce, hits, finite, out[3].detach()[el:el + b * K * Ts].view(b, K, Ts) if dense else None))
        row, el = row + b * Ts, el + b * K * Ts
    return stats
