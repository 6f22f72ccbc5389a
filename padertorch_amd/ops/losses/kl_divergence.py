"""The pairwise KL divergence between diagonal Gaussian posteriors and the components of a Gaussian (mixture) prior on the MI355X
(reference: ``padertorch/ops/losses/kl_divergence.py:17-60``) on the kernels of ``csrc/gauss_kl.hip``.

    gaussian_kl_divergence(q: Normal (B1, ..., BN, D), p: Normal | MultivariateNormal (K1, ..., KN, D)) -> (B1, ..., BN, K1, ..., KN)

The reference composes it from an ``inverse()`` of the ``scale_tril`` factors, a ``[K, B, D]`` difference tensor and a batched matmul;
here the components are prepared once (``L = scale_tril^-1`` by forward substitution), a row-owning kernel streams them past the
posteriors it keeps in registers, and the backward is a row-owning kernel (``dloc``, ``dscale`` of ``q``), a component-owning kernel
with fixed-order partials and a component finish (``dloc``, ``dscale`` / ``dscale_tril`` of ``p``).  Nothing of size ``B K D`` is
written, no atomics, no host reads: forward + backward capture into a graph.

Departure from the reference: only the lower triangle of ``scale_tril`` is read, and its gradient is zero above the diagonal.  (The
reference's autograd goes through a general ``inverse()``: the same lower triangle, and values without meaning above it.)

fp32 on the GPU only; ``D <= 64`` (``ptmi_gkl_max_features``), ``NotImplementedError`` beyond and for other dtypes.  ``q`` must be a
``Normal``: a full-covariance posterior is not covered (as in the reference).
"""
import torch
from torch.autograd.function import once_differentiable
from torch.distributions import MultivariateNormal, Normal

from ... import _lib
from .. import library  # noqa: F401  (registers torch.ops.ptmi.gkl_*)

__all__ = [
    'gaussian_kl_divergence',
]

#: rows a row-owning workgroup owns / rows of one (component, split) workgroup of the backward (``ptmi_gkl_row_tile()`` /
#: ``ptmi_gkl_split_rows()``): what the tests put B around
kGklBM, kGklSplitRows = 64, 1024


class _GaussianKlFn(torch.autograd.Function):
    """``(mu, sigma [B, D], m [K, D], scale [K, D] or scale_tril [K, D, D]) -> kl [B, K]``."""

    @staticmethod
    def forward(ctx, mu, sigma, m, scale):
        L, c, logdet = torch.ops.ptmi.gkl_prepare(scale, mu.shape[1])
        ctx.save_for_backward(mu, sigma, m, scale, L, c)
        return torch.ops.ptmi.gkl_forward(mu, sigma, m, scale, L, c, logdet)

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        return torch.ops.ptmi.gkl_backward(*ctx.saved_tensors, g.contiguous())


def gaussian_kl_divergence(q, p):
    """
    Args:
        q: Normal posterior distributions (B1, ..., BN, D)
        p: (Multivariate) Normal prior distributions (K1, ..., KN, D)

    Returns: kl between all posteriors in batch and all components
        (B1, ..., BN, K1, ..., KN)

    """
    assert isinstance(q, Normal), type(q)
    batch_shape = q.loc.shape[:-1]
    D = q.loc.shape[-1]
    component_shape = p.loc.shape[:-1]
    assert p.loc.shape[-1] == D, (p.loc.shape[-1], D)
    if isinstance(p, MultivariateNormal):
        p_scale = p.scale_tril.contiguous().view(-1, D, D)
    elif isinstance(p, Normal):
        p_scale = p.scale.contiguous().view(-1, D)
    else:
        raise ValueError
    operands = (q.loc.contiguous().view(-1, D), q.scale.contiguous().view(-1, D), p.loc.contiguous().view(-1, D), p_scale)
    _lib.require_gpu(*operands)
    for x in operands:
        if x.dtype != torch.float32:
            raise NotImplementedError(f'gaussian_kl_divergence: float32 only, got {x.dtype}')
    return _GaussianKlFn.apply(*operands).view(*batch_shape, *component_shape)
