"""The One-and-Rest PIT loss and flag head on the HIP kernels of ``csrc/orpit.hip``
(``padertorch/contrib/examples/source_separation/or_pit/model.py:11-98,187-218,319-350``).

    or_pit_iterations(estimates, targets)
        the batched loss of ``OneAndRestPIT.review``: ``estimates`` a list of ``[B, 2, T]`` (one per iteration), ``targets [B, K, T]``
        -> ``(losses [iterations, B], choices [iterations, B] int32)``.  Per iteration ONE streaming pass over the rows
        (``td_rect_stats``), one tiny selection launch (``orpit_select``: the first minimum, the alive mask and the gradient's
        coefficients stay on the device) and, backward, one more streaming pass (``td_rect_lincomb``).  No host value is read and no
        index table is built on the host: a step can be captured in a graph.
    one_and_rest_permutation_invariant_loss(inputs, targets, loss_fn, fill_missing_with_zeros=False)
        the reference's function of one example, same arguments and return values
    flag_head(additional, weight, bias, mode='mean', mask=None, encoded=None)
        ``additional [B, A, E]`` -> ``(flag [B], pre [B, E])``; the weighted modes read ``mask [K, B, N, E]`` and ``encoded [B, N, E]``
        directly, ``mask * encoded`` is never formed

Targets get no gradient: a target that requires grad raises.  fp32 on the GPU only: other dtypes raise ``NotImplementedError``, CPU
tensors the "no CPU fallback" error.
"""
import torch
from torch.autograd.function import once_differentiable

from .. import _lib
from . import library  # noqa: F401  (registers torch.ops.ptmi.*)
from .losses import regression

__all__ = ['or_pit_iterations', 'one_and_rest_permutation_invariant_loss', 'flag_head', 'FLAG_MODES']

#: flag reduction -> the mask row whose energy weights the frames (None: the plain mean)
FLAG_MODES = {'mean': None, 'est-weighted-mean': 0, 'res-weighted-mean': 1}


def _check(name, *tensors):
    for t in tensors:                   # (the dtype first: a float64 tensor is refused for what it is, wherever it lives)
        if t is not None and t.dtype != torch.float32:
            raise NotImplementedError(f'{name}: float32 only, got {t.dtype}')
    _lib.require_gpu(*tensors)


def _time_rows(x):
    return x if x.stride(-1) == 1 or x.shape[-1] == 1 else x.contiguous()


def _signals(name, est, tgt):
    _check(name, est, tgt)
    if est.dim() != 3 or tgt.dim() != 3 or est.shape[0] != tgt.shape[0] or est.shape[2] != tgt.shape[2] or est.numel() == 0:
        raise ValueError(f'{name}: estimates [B, M, T] and targets [B, K, T], got {tuple(est.shape)}, {tuple(tgt.shape)}')
    if est.shape[1] > 8 or tgt.shape[1] > 8:
        raise NotImplementedError(f'{name}: at most 8 rows a side, got {est.shape[1]} and {tgt.shape[1]}')
    if tgt.requires_grad:
        raise ValueError(f'{name}: the targets get no gradient, but they require one')
    return _time_rows(est), (_time_rows(tgt) if tgt.shape[1] else None)


class _IterationFn(torch.autograd.Function):
    """Kernels: ``td_rect_stats`` + ``orpit_select``; ``td_rect_lincomb`` (saves the signals and the coefficients)."""

    @staticmethod
    def forward(ctx, est, tgt, gram, alive):
        stats, new_gram = torch.ops.ptmi.td_rect_stats(est, tgt, gram is None)
        loss, choice, alive_out, a, b = torch.ops.ptmi.orpit_select(stats, new_gram if gram is None else gram, alive, est.shape[2])
        ctx.save_for_backward(est, tgt, a, b)
        ctx.mark_non_differentiable(choice, alive_out, new_gram)
        return loss, choice, alive_out, new_gram

    @staticmethod
    @once_differentiable
    def backward(ctx, g, _choice, _alive, _gram):
        est, tgt, a, b = ctx.saved_tensors
        return torch.ops.ptmi.td_rect_lincomb(est, tgt, g.contiguous(), a, b), None, None, None


class _RectStatsFn(torch.autograd.Function):
    """``td_rect_stats`` with its adjoint w.r.t. the estimates: ``d e_m = 2 g_See[m] e_m + sum_j g_C[m][j] t_j`` (``td_rect_lincomb``)."""

    @staticmethod
    def forward(ctx, est, tgt):
        stats, gram = torch.ops.ptmi.td_rect_stats(est, tgt, True)
        ctx.save_for_backward(est, tgt)
        ctx.mark_non_differentiable(gram)
        return stats, gram

    @staticmethod
    @once_differentiable
    def backward(ctx, g, _gram):
        est, tgt = ctx.saved_tensors
        B, M, _ = est.shape
        K = 0 if tgt is None else tgt.shape[1]
        g = g.to(torch.float32)
        a, b = (2 * g[:, M * K:]).contiguous(), g[:, :M * K].reshape(B, M, K).contiguous()
        return torch.ops.ptmi.td_rect_lincomb(est, tgt, None, a, b), None


def or_pit_iterations(estimates, targets):
    """``estimates``: the ``[B, 2, T]`` outputs of the iterations in order, ``targets [B, K, T]`` (``K >= 0``).  Iteration ``k`` sees
    the targets no earlier iteration has chosen (``R = max(K - k, 0)`` of them) and restates
    ``one_and_rest_permutation_invariant_loss(..., log_mse_loss, fill_missing_with_zeros=True)``.  Returns ``(losses [iterations, B]
    float32, choices [iterations, B] int32)``; a choice is the index into ``targets`` (``-1``: no target was left)."""
    B, K = targets.shape[0], targets.shape[1]
    alive = torch.ones((B, K), dtype=torch.int32, device=targets.device)
    gram, losses, choices = None, [], []
    for est in estimates:
        est, tgt = _signals('or_pit_iterations', est, targets)
        if est.shape[1] != 2:
            raise ValueError(f'or_pit_iterations: two estimates per iteration, got {tuple(est.shape)}')
        loss, choice, alive, new_gram = _IterationFn.apply(est, tgt, gram, alive)
        gram = new_gram if gram is None else gram          # the targets' Gram matrix: once per step
        losses.append(loss)
        choices.append(choice)
    return torch.stack(losses), torch.stack(choices)


def one_and_rest_permutation_invariant_loss(inputs, targets, loss_fn, fill_missing_with_zeros=False):
    """The reference's function (``or_pit/model.py:11-98``): ``inputs [2, T]``, ``targets [K, T]`` -> ``(loss, perm)``, the loss of
    ``inputs[0]`` against one target plus ``1 / (K - 1)`` times the loss of ``inputs[1]`` against the sum of the others, minimised
    over the choice; ``perm`` is that target's index.  ``loss_fn``: a loss of ``ops.losses.regression`` (or a ``functools.partial``
    of one with keyword arguments).  ``log_mse_loss`` runs through ``orpit_select``; the other losses are evaluated with their
    closed forms on the same statistics; anything else raises ``NotImplementedError``."""
    spec = regression.resolve(loss_fn)
    if spec is None:
        raise NotImplementedError(f'one_and_rest_permutation_invariant_loss: {loss_fn!r} is no loss of ops.losses.regression')
    assert inputs.shape[0] == 2
    K = targets.shape[0]
    if K == 0 and not fill_missing_with_zeros:
        return inputs.new_zeros(1), 0
    if K == 1 and not fill_missing_with_zeros:
        return loss_fn(inputs[0], targets[0]), 0
    if inputs.dim() != 2 or targets.dim() != 2:
        raise NotImplementedError(f'one_and_rest_permutation_invariant_loss: [2, T] and [K, T] signals, got {tuple(inputs.shape)}, '
                                  f'{tuple(targets.shape)}')
    est, tgt = _signals('one_and_rest_permutation_invariant_loss', inputs[None], targets[None])
    rows_fn, reduction, kwargs = spec
    if rows_fn is regression._rows_log_mse and reduction == 'sum' and not kwargs:
        alive = torch.ones((1, K), dtype=torch.int32, device=est.device)
        loss, choice, _, _ = _IterationFn.apply(est, tgt, None, alive)
        return loss[0], (choice[0].to(torch.int64) if K >= 2 else 0)
    if kwargs.get('offset_invariant'):
        raise NotImplementedError('one_and_rest_permutation_invariant_loss: offset_invariant needs the signals\' sums, which the '
                                  'rectangular statistics do not carry')
    stats, gram = _RectStatsFn.apply(est, tgt)
    n = torch.full((), float(est.shape[2]), dtype=torch.float64, device=est.device)
    C, see, G = stats[0, :2 * K].reshape(2, K), stats[0, 2 * K:], (gram[0] if K else None)
    zero = torch.zeros((), dtype=torch.float64, device=est.device)

    def rows(see_, stt, set_):
        if rows_fn == 'aggregated':
            return regression._aggregated(see_, stt, set_, kwargs.get('soft_sdr_max'))
        return rows_fn(dict(see=see_, stt=stt, set=set_, se=zero, st=zero, n=n), **kwargs)

    if K < 2:       # filled with zeros: the loss function's own reduction over the two rows
        stt = torch.stack([G[0, 0], zero]) if K else torch.zeros(2, dtype=torch.float64, device=est.device)
        set_ = torch.stack([C[0, 0], zero]) if K else stt
        if rows_fn == 'aggregated':
            return rows(see.sum(), stt.sum(), set_.sum()).to(inputs.dtype), 0
        both = rows(see, stt, set_)
        return (both.sum() if reduction == 'sum' else both.mean()).to(inputs.dtype), 0
    rest = 1 - torch.eye(K, dtype=torch.float64, device=est.device)
    candidates = rows(see[0], torch.diagonal(G), C[0]) + rows(see[1], ((rest @ G) * rest).sum(1), rest @ C[1]) / (K - 1)
    loss, perm = torch.min(candidates, dim=0)
    return loss.to(inputs.dtype), perm


class _FlagFn(torch.autograd.Function):
    """Kernels: ``orpit_flag_forward``; ``orpit_flag_backward`` (saves the inputs, ``pre``, the frame weights and two doubles a row)."""

    @staticmethod
    def forward(ctx, additional, weight, bias, mask, encoded, k):
        additional = additional.contiguous()
        w_, b_ = weight.reshape(-1).contiguous(), bias.reshape(-1).contiguous()
        mask = None if mask is None else mask.contiguous()
        encoded = None if encoded is None else encoded.contiguous()
        pre, flag, w, stat = torch.ops.ptmi.orpit_flag_forward(additional, w_, b_, mask, encoded, k)
        ctx.save_for_backward(additional, w_, mask, encoded, pre, flag, w, stat)
        ctx.k, ctx.shapes = k, (weight.shape, bias.shape)
        ctx.set_materialize_grads(False)
        return flag, pre

    @staticmethod
    @once_differentiable
    def backward(ctx, gflag, gpre):
        additional, w_, mask, encoded, pre, flag, w, stat = ctx.saved_tensors
        if gflag is None and gpre is None:
            return None, None, None, None, None, None
        gflag = torch.zeros_like(flag) if gflag is None else gflag.contiguous()
        gpre = None if gpre is None else gpre.contiguous()
        dadd, dparams, dmask, denc = torch.ops.ptmi.orpit_flag_backward(gflag, gpre, flag, stat, pre, w, additional, w_, mask, encoded, ctx.k)
        A = w_.numel()
        need = ctx.needs_input_grad
        return (dadd if need[0] else None, dparams[:A].view(ctx.shapes[0]) if need[1] else None,
                dparams[A:].view(ctx.shapes[1]) if need[2] else None, dmask if need[3] else None, denc if need[4] else None, None)


def flag_head(additional, weight, bias, mode='mean', mask=None, encoded=None):
    """``additional [B, A, E]`` (``mask_head``'s second output), ``weight`` (``A`` values: ``torch.nn.Linear(A, 1).weight``), ``bias``
    (one value) -> ``(flag [B], pre [B, E])``: ``pre[b, e] = bias + sum_a weight[a] additional[b, a, e]`` and

        ``mean``                                     ``flag = sigmoid(mean_e pre)``
        ``res-weighted-mean`` / ``est-weighted-mean``  ``flag = sigmoid(sum_e pre w / sum_e w)``, ``w[b, e] = mean_n (mask[k, b, n, e]
                                                     encoded[b, n, e])^2`` with ``k = 1`` / ``k = 0``

    ``mask [K, B, N, E]``, ``encoded [B, N, E]`` or None when the mask is the estimate itself (a separator built with ``mask=False``).
    There is no epsilon: a silent stream gives ``0 / 0`` as in the reference.  Differentiable in every tensor."""
    if mode not in FLAG_MODES:
        raise ValueError(f'flag_head: mode one of {sorted(FLAG_MODES)}, got {mode!r}')
    k = FLAG_MODES[mode]
    if k is None:
        mask = encoded = None
    elif mask is None:
        raise ValueError(f'flag_head: mode {mode!r} needs the mask')
    _check('flag_head', additional, weight, bias, mask, encoded)
    if additional.dim() != 3 or additional.numel() == 0 or weight.numel() != additional.shape[1] or bias.numel() != 1:
        raise ValueError(f'flag_head: additional [B, A, E] with A weights and one bias, got {tuple(additional.shape)}, '
                         f'{tuple(weight.shape)}, {tuple(bias.shape)}')
    if mask is not None:
        B, _, E = additional.shape
        if mask.dim() != 4 or mask.shape[0] <= k or (mask.shape[1], mask.shape[3]) != (B, E) or \
                (encoded is not None and tuple(encoded.shape) != tuple(mask.shape[1:])):
            raise ValueError(f'flag_head: mask [K > {k}, {B}, N, {E}] and encoded [{B}, N, {E}], got {tuple(mask.shape)}, '
                             f'{None if encoded is None else tuple(encoded.shape)}')
    return _FlagFn.apply(additional, weight, bias, mask, encoded, 0 if k is None else k)
