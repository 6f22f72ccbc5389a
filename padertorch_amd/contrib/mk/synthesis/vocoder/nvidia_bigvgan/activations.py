"""``Snake`` and ``SnakeBeta`` (reference: ``nvidia_bigvgan/activations.py``): constructor, parameter names and ``state_dict`` of the
reference; the forward is the HIP kernel (``padertorch_amd.ops.anti_alias.snake``), differentiable in ``x`` and the parameters.

Inside an :class:`~.alias_free_activation.Activation1d` these modules are not called: their parameters go to the fused launch."""
import torch
from torch import nn

from ......ops import anti_alias

__all__ = ['Snake', 'SnakeBeta']


def _parameter(in_features, alpha, alpha_trainable, alpha_logscale):
    # log scale starts at exp(0) = 1 whatever `alpha` is, as in the reference
    init = torch.zeros(in_features) * alpha if alpha_logscale else torch.ones(in_features) * alpha
    return nn.Parameter(init, requires_grad=alpha_trainable)


class Snake(nn.Module):
    """``x + sin^2(alpha x) / alpha`` per channel of ``[B, C, T]``."""

    def __init__(self, in_features, alpha=1.0, alpha_trainable=True, alpha_logscale=False):
        super().__init__()
        self.in_features = in_features
        self.alpha_logscale = alpha_logscale
        self.alpha = _parameter(in_features, alpha, alpha_trainable, alpha_logscale)
        self.no_div_by_zero = 0.000000001

    def kernel_parameters(self):
        """``(alpha, beta)`` as the kernel takes them: ``beta=None`` means the magnitude parameter is ``alpha`` itself."""
        return self.alpha, None

    def forward(self, x):
        return anti_alias.snake(x, *self.kernel_parameters(), alpha_logscale=self.alpha_logscale)


class SnakeBeta(nn.Module):
    """``x + sin^2(alpha x) / beta`` per channel of ``[B, C, T]``: frequency and magnitude as separate parameters."""

    def __init__(self, in_features, alpha=1.0, alpha_trainable=True, alpha_logscale=False):
        super().__init__()
        self.in_features = in_features
        self.alpha_logscale = alpha_logscale
        self.alpha = _parameter(in_features, alpha, alpha_trainable, alpha_logscale)
        self.beta = _parameter(in_features, alpha, alpha_trainable, alpha_logscale)
        self.no_div_by_zero = 0.000000001

    def kernel_parameters(self):
        return self.alpha, self.beta

    def forward(self, x):
        return anti_alias.snake(x, *self.kernel_parameters(), alpha_logscale=self.alpha_logscale)
