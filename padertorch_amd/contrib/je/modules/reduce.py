"""The poolings over time of ``padertorch/contrib/je/modules/reduce.py`` on the kernels of ``csrc/seq_pool.hip``: ``Sum``, ``Mean``,
``Max``, ``TakeLast`` and ``AutoPool`` with the reference's constructors, called as ``module(x, seq_len=None)``.  Each call is one
launch of ``ops.seq_pool.seq_pool`` (no mask tensor, no multiply) that reads ``x`` in place whatever its strides; see that module for
the semantics, the accepted forms of ``seq_len`` and the one departure (a NaN BEHIND the length does not reach the result).  ``Max``
returns ``(values, indices)`` as the reference's ``x.max(axis)`` does.  fp32 on the GPU only.
"""
import torch
from torch import nn

from ....ops.seq_pool import seq_pool

__all__ = ['Sum', 'Mean', 'Max', 'TakeLast', 'AutoPool']


class Sum(nn.Module):
    mode = 'sum'

    def __init__(self, axis=-1, keepdims=False):
        self.axis = axis
        self.keepdims = keepdims
        super().__init__()

    def forward(self, x, seq_len=None):
        return seq_pool(x, seq_len, self.axis, self.mode, self.keepdims)


class Mean(Sum):
    mode = 'mean'


class Max(Sum):
    mode = 'max'


class TakeLast(Sum):
    mode = 'last'


class AutoPool(nn.Module):
    """``sum_t softmax_t(alpha x) x`` over the last axis of ``x [B, n_classes, T]`` (https://arxiv.org/abs/1804.10070);
    ``trainable``: ``alpha`` is a parameter ``[n_classes, 1]``."""

    def __init__(self, n_classes, alpha=1., trainable=False):
        super().__init__()
        self.trainable = trainable
        if trainable:
            self.alpha = nn.Parameter(alpha * torch.ones((n_classes, 1)))
        else:
            self.alpha = alpha

    def forward(self, x, seq_len=None):
        return seq_pool(x, seq_len, -1, 'autopool', False, alpha=self.alpha)
