"""The mask estimator's loss on the HIP kernels of ``csrc/mask_loss.hip``
(``padertorch/contrib/jensheit/mask_estimator_example/model.py:128-237``, ``add_losses``).

    mask_bce_loss(logits, target, num_frames=None, power=None, reduction='mean') -> (pooled [B], weighted [B] or None)

``logits, target [B, C, T, F]``: per example ``b`` over its ``n_b = C num_frames[b] F`` elements the binary cross-entropy on logits
``l = max(x, 0) - x t + log1p(exp(-|x|))`` pooled by ``reduction`` (``mean``, ``median`` - torch's lower median -, ``min``, ``max``) and,
with ``power`` (the observation's complex64 STFT, or real weights), ``sum l w / sum w`` from the same pass.  What lies behind
``num_frames[b]`` is never read.  The reference computes this per example with ``F.binary_cross_entropy_with_logits(reduction='none')``,
``TORCH_POOLING_FN_MAP[reduction]`` and ``weight_loss``; here the whole padded batch is one call, strided views are consumed in place,
and ``num_frames`` stays on the device: a captured graph serves every length pattern of a padded shape.

Differentiable in ``logits`` only: ``target`` and ``power`` get no gradient, and one that requires a gradient raises.  fp32 on the GPU
only: other dtypes raise ``ValueError``, CPU tensors the "no CPU fallback" error.
"""
import torch
from torch.autograd.function import once_differentiable

from .. import _lib
from . import library  # noqa: F401  (registers torch.ops.ptmi.*)

__all__ = ['mask_bce_loss', 'MASK_REDUCTIONS']

#: pooling name -> the kernels' code
MASK_REDUCTIONS = {'mean': 0, 'median': 1, 'min': 2, 'max': 3}


class _MaskLossFn(torch.autograd.Function):
    """Kernels: ``mask_loss_forward`` (stats, selection, finalize); ``mask_loss_backward`` (saves the inputs, the sums and the selected
    key with its multiplicity - the element losses are recomputed, not stored)."""

    @staticmethod
    def forward(ctx, logits, target, power, num_frames, reduction):
        pooled, weighted, stat, sel = torch.ops.ptmi.mask_loss_forward(logits, target, power, num_frames, reduction)
        ctx.save_for_backward(logits, target, power, num_frames, stat, sel)
        ctx.reduction = reduction
        ctx.set_materialize_grads(False)
        if weighted is None:
            return pooled, None
        return pooled, weighted

    @staticmethod
    @once_differentiable
    def backward(ctx, g_pooled, g_weighted):
        logits, target, power, num_frames, stat, sel = ctx.saved_tensors
        if g_pooled is None and g_weighted is None:
            return None, None, None, None, None
        g_pooled = None if g_pooled is None else g_pooled.contiguous()
        g_weighted = None if g_weighted is None or power is None else g_weighted.contiguous()
        dlogits = torch.ops.ptmi.mask_loss_backward(logits, target, power, num_frames, g_pooled, g_weighted, stat, sel, ctx.reduction)
        return dlogits, None, None, None, None          # no gradient for the target, the power or the lengths


def mask_bce_loss(logits, target, num_frames=None, power=None, reduction='mean'):
    """``logits, target [B, C, T, F]`` float32 with unit stride on ``F`` (any other strides: the estimator's views are read in place);
    ``num_frames``: None (full length), a host list, or an int32 device tensor ``[B]`` (used as it is); ``power``: None, complex64
    ``[B, C, T, F]`` (the kernel forms ``re^2 + im^2``) or float32 weights.  Returns ``(pooled [B], weighted [B] or None)``.

    ``median`` is the element of rank ``(n_b - 1) // 2``; a NaN element makes ``pooled`` NaN; ``sum w == 0`` makes ``weighted`` NaN.
    Backward: ``mean`` spreads ``g / n_b``; ``median`` / ``min`` / ``max`` give ``g / m_b`` to each of the ``m_b`` elements whose loss
    equals the pooled value (torch's even split among ties); behind ``num_frames`` the gradient is exactly zero."""
    name = 'mask_bce_loss'
    if reduction not in MASK_REDUCTIONS:
        raise ValueError(f'{name}: reduction one of {sorted(MASK_REDUCTIONS)}, got {reduction!r}')
    if not torch.is_tensor(logits) or not torch.is_tensor(target) or logits.dim() != 4 or logits.shape != target.shape \
            or logits.numel() == 0:
        raise ValueError(f'{name}: logits and target [B, C, T, F] of one shape, got '
                         f'{tuple(logits.shape) if torch.is_tensor(logits) else type(logits)}, '
                         f'{tuple(target.shape) if torch.is_tensor(target) else type(target)}')
    if logits.dtype != torch.float32 or target.dtype != torch.float32:
        raise ValueError(f'{name}: float32 logits and target, got {logits.dtype}, {target.dtype}')
    B, C, T, F = logits.shape
    if power is not None:
        if not torch.is_tensor(power) or power.shape != logits.shape:
            raise ValueError(f'{name}: power {tuple(logits.shape)} like the logits, got '
                             f'{tuple(power.shape) if torch.is_tensor(power) else type(power)}')
        if power.dtype not in (torch.float32, torch.complex64):
            raise ValueError(f'{name}: power float32 or complex64, got {power.dtype}')
    _lib.require_gpu(logits, target, power)
    for what, t in (('logits', logits), ('target', target), ('power', power)):
        if t is None:
            continue
        if t.device != logits.device:
            raise ValueError(f'{name}: {what} on {t.device}, logits on {logits.device}')
        if F > 1 and t.stride(3) != 1:
            raise ValueError(f'{name}: {what} needs unit stride on F, got shape {tuple(t.shape)} with strides {tuple(t.stride())}')
    if target.requires_grad or (power is not None and power.requires_grad):
        raise ValueError(f'{name}: target and power get no gradient, but one requires it')
    if B > 65535 or C * T * F >= 2 ** 31:
        raise ValueError(f'{name}: at most 65535 examples of fewer than 2^31 elements, got {tuple(logits.shape)}')
    if num_frames is not None:
        if torch.is_tensor(num_frames) and num_frames.is_cuda:
            if num_frames.dtype != torch.int32 or tuple(num_frames.shape) != (B,) or num_frames.device != logits.device:
                raise ValueError(f'{name}: num_frames int32 [{B}] on {logits.device}, got {num_frames.dtype} {tuple(num_frames.shape)} on '
                                 f'{num_frames.device}')
            num_frames = num_frames.contiguous()
        else:
            host = [int(n) for n in (num_frames.tolist() if torch.is_tensor(num_frames) else num_frames)]
            if len(host) != B or any(not 0 <= n <= T for n in host):
                raise ValueError(f'{name}: one length in [0, {T}] per example ({B}), got {host}')
            num_frames = None if all(n == T for n in host) else _lib.host_to_device(host, torch.int32, logits.device)
    pooled, weighted = _MaskLossFn.apply(logits, target, power, num_frames, MASK_REDUCTIONS[reduction])
    return pooled, weighted
