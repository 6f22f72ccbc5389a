"""The angular-margin softmax head (``padertorch/contrib/tcl/speaker_embeddings/loss.py:64-103``) and the ``nn.BatchNorm1d(E,
affine=False)`` in front of it (``dvectors.py``) on the kernels of ``csrc/aam_softmax.hip``.

    angular_softmax_loss(embeddings [B, E] or [E], weight [C, E], labels [B], loss_type='aam', s=None, m=None, eps=1e-7,
                         reduce='mean', check=True)  ->  -mean(L) (a scalar) or -L [B]
    batch_norm_rows(x [B, E], running_mean, running_var, num_batches_tracked, training, momentum, eps) -> y [B, E]

With ``W_hat`` / ``e_hat`` the row-normalised operands (``x / max(||x||, 1e-12)``) and ``cos = e_hat W_hat^T``:

    n_b   'aam'         s (cos_y - m)                                                    defaults s = 30, m = 0.2
          'arcface'     s cos(acos(clamp(cos_y, -1 + eps, 1 - eps)) + m)                  s = 64, m = 0.5
          'sphereface'  s cos(m acos(clamp(cos_y, -1 + eps, 1 - eps)))                    s = 64, m = 1.35
    L_b = n_b - log(exp(n_b) + sum_{c != y} exp(s cos[b, c]))

``weight`` is normalised IN PLACE, as the reference's ``module.weight.data = normalize(...)`` does, so its gradient is the one with respect
to the normalised rows (no projection); the embedding's gradient goes through its normalisation; the clamp passes no gradient outside its
range.  The launch list of a call - nothing in it writes ``[B, C]``:

    forward    aam_prepare (rows of W and e, one launch) | aam_forward (class tiles -> partials [tiles, B]) | aam_finish (rows) | aam_mean
    backward   aam_dw (class tiles, streams the batch) | aam_de (row tiles x class ranges) | aam_de_finish (rows)

``labels``: an int32 / int64 CUDA tensor is read by the kernels only, so forward + backward capture into a graph that serves other labels;
a list, numpy array or CPU tensor is uploaded once.  ``check=True`` keeps the reference's host assertions on the labels (a host read);
``check=False`` is the capturable call: a label outside ``[0, C)`` then makes that row's loss NaN, gives it no gradient and indexes nothing.

Departure from the reference: the log-sum-exp carries a running maximum, so where the reference's ``exp(s cos)`` overflows fp32
(``s cos`` near 88) this stays finite.  fp32 on the GPU only, ``E <= ptmi_aam_max_features()`` (512).
"""
import torch
from torch.autograd.function import once_differentiable

from .. import _lib
from . import library  # noqa: F401  (registers torch.ops.ptmi.aam_*, batch_norm_rows_*)
from .gru import device_lengths

__all__ = ['angular_softmax_loss', 'batch_norm_rows', 'max_features', 'LOSS_TYPES', 'DEFAULTS', 'kAamBN', 'kAamBM']

LOSS_TYPES = {'aam': 0, 'arcface': 1, 'sphereface': 2}
#: (s, m) of the reference's constructor per loss type
DEFAULTS = {'aam': (30.0, 0.2), 'arcface': (64.0, 0.5), 'sphereface': (64.0, 1.35)}


#: classes a workgroup owns / batch rows of a streamed tile (``ptmi_aam_class_tile()`` / ``ptmi_aam_row_tile()``): what the tests put C
#: and B around
kAamBN, kAamBM = 32, 64


def max_features():
    """``ptmi_aam_max_features()``: the largest embedding size the kernels stage (a host function of the library: no GPU needed)."""
    return int(_lib.load().ptmi_aam_max_features())


class _AamFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, e, weight, labels, loss_type, s, m, eps, mean):
        e_hat, e_rnorm = torch.ops.ptmi.aam_prepare(weight.detach(), e)
        w_hat = weight.detach()
        rows, lse, n, dn, total = torch.ops.ptmi.aam_forward(w_hat, e_hat, labels, loss_type, s, m, eps, mean)
        ctx.save_for_backward(w_hat, e_hat, e_rnorm, labels, lse, n, dn)
        ctx.cfg = (s, mean)
        return total if mean else rows

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        w_hat, e_hat, e_rnorm, labels, lse, n, dn = ctx.saved_tensors
        s, mean = ctx.cfg
        dw, de = torch.ops.ptmi.aam_backward(w_hat, e_hat, e_rnorm, labels, lse, n, dn, g.contiguous(), mean, s, ctx.needs_input_grad[1],
                                             ctx.needs_input_grad[0])
        return de, dw, None, None, None, None, None, None


def angular_softmax_loss(embeddings, weight, labels, loss_type='aam', s=None, m=None, eps=1e-7, reduce='mean', check=True):
    """The loss of the module docstring; ``weight`` (contiguous) comes back row-normalised."""
    loss_type = loss_type.lower()
    if loss_type not in LOSS_TYPES:
        raise ValueError(f'angular_softmax_loss: loss_type one of {sorted(LOSS_TYPES)}, got {loss_type!r}')
    s0, m0 = DEFAULTS[loss_type]
    s, m = float(s if s else s0), float(m if m else m0)
    one_row = embeddings.dim() == 1
    if one_row:
        embeddings = embeddings[None, :]
    if embeddings.dim() != 2 or weight.dim() != 2 or embeddings.shape[1] != weight.shape[1] or weight.shape[0] < 2 or embeddings.shape[0] < 1:
        raise ValueError(f'angular_softmax_loss: embeddings [B, E] and weight [C, E] with C >= 2, got {tuple(embeddings.shape)}, '
                         f'{tuple(weight.shape)}')
    if embeddings.shape[1] > max_features():
        raise NotImplementedError(f'angular_softmax_loss: {embeddings.shape[1]} features; the kernels stage up to {max_features()} '
                                  f'(ptmi_aam_max_features)')
    for t in (embeddings, weight):
        if t.dtype != torch.float32:
            raise NotImplementedError(f'angular_softmax_loss: float32 only, got {t.dtype}')
    _lib.require_gpu(embeddings, weight)
    if not weight.is_contiguous():
        raise ValueError('angular_softmax_loss: weight is normalised in place and has to be contiguous')
    B, C = embeddings.shape[0], weight.shape[0]
    if not (torch.is_tensor(labels) and labels.is_cuda):
        assert len(labels) == B, (len(labels), B)
    labels = device_lengths(labels, B, embeddings.device)
    if check:                                                   # loss.py:75-77 (host reads)
        assert torch.min(labels) >= 0
        assert torch.max(labels) < C
    return _AamFn.apply(embeddings.contiguous(), weight, labels, LOSS_TYPES[loss_type], s, m, float(eps), reduce == 'mean')


class _BatchNormRowsFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, running_mean, running_var, num_batches_tracked, training, momentum, eps):
        y, stats = torch.ops.ptmi.batch_norm_rows_forward(x, running_mean, running_var, num_batches_tracked, training, momentum, eps)
        ctx.save_for_backward(x, stats)
        ctx.training = training
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        x, stats = ctx.saved_tensors
        return torch.ops.ptmi.batch_norm_rows_backward(g.contiguous(), x, stats, ctx.training), None, None, None, None, None, None


def batch_norm_rows(x, running_mean=None, running_var=None, num_batches_tracked=None, training=True, momentum=0.1, eps=1e-5):
    """``nn.BatchNorm1d(E, affine=False)`` on ``x [B, E]``: in training the batch statistics (fp64 column sums in a fixed order, biased
    variance) and the buffers' update (unbiased variance, ``momentum``, counter + 1) in one launch; in evaluation the running statistics."""
    if x.dim() != 2 or x.numel() == 0:
        raise ValueError(f'batch_norm_rows: x [B, E], got {tuple(x.shape)}')
    for t in (x, running_mean, running_var):
        if t is not None and t.dtype != torch.float32:
            raise NotImplementedError(f'batch_norm_rows: float32 only, got {t.dtype}')
    _lib.require_gpu(x, running_mean, running_var, num_batches_tracked)
    if momentum is None:
        raise NotImplementedError('batch_norm_rows: momentum=None (the cumulative average) is not built')
    if training and x.shape[0] < 2:
        raise ValueError(f'batch_norm_rows: expected more than 1 value per channel when training, got input size {tuple(x.shape)}')
    if not training and (running_mean is None or running_var is None):
        raise ValueError('batch_norm_rows: evaluation needs the running statistics')
    return _BatchNormRowsFn.apply(x.contiguous(), running_mean, running_var, num_batches_tracked, bool(training), float(momentum), float(eps))
