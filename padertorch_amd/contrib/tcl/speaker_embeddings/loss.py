"""``AngularPenaltySMLoss`` of ``padertorch/contrib/tcl/speaker_embeddings/loss.py`` on the fused head of ``csrc/aam_softmax.hip``:
the last fully connected layer and the classification loss in one, with the reference's constructor, its defaults per loss type and
``fc = nn.Linear(in_features, out_features, bias=False)`` as the parameter holder, so ``fc.weight`` loads.  See ``ops.aam_softmax`` for
the formulas, the launch list and the one departure (a stabilised log-sum-exp)."""
import torch

from .... import base
from ....ops.aam_softmax import DEFAULTS, angular_softmax_loss

__all__ = ['AngularPenaltySMLoss']


class AngularPenaltySMLoss(base.Module):
    """Angular penalty softmax losses ``'arcface'`` (https://arxiv.org/abs/1801.07698), ``'sphereface'``
    (https://arxiv.org/abs/1704.08063) and ``'aam'`` (https://arxiv.org/abs/1801.05599).

    ``forward(embeddings [B, E] or [E], labels [B]) -> -mean(L)`` (``reduce='mean'``) or ``-L [B]``.  As in the reference the call
    normalises ``fc.weight`` in place.  ``check=False`` skips the reference's host assertions on the labels (the capturable call)."""

    def __init__(self, in_features, out_features, loss_type='aam', eps=1e-7, s=None, m=None, reduce='mean'):
        super().__init__()
        loss_type = loss_type.lower()
        assert loss_type in ['arcface', 'sphereface', 'aam']
        s0, m0 = DEFAULTS[loss_type]
        self.s = s0 if not s else s
        self.m = m0 if not m else m
        self.loss_type = loss_type
        self.in_features = in_features
        self.out_features = out_features
        self.fc = torch.nn.Linear(in_features, out_features, bias=False)
        self.eps = eps
        self.reduce = reduce

    def forward(self, embeddings, labels, check=True):
        return angular_softmax_loss(embeddings, self.fc.weight, labels, self.loss_type, self.s, self.m, self.eps, self.reduce, check)
