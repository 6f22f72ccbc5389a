"""``gaussian_kl_divergence`` without a GPU: where it is reachable, what it refuses, the limits the library exports."""
import pytest
import torch
from torch.distributions import Laplace, MultivariateNormal, Normal

import padertorch_amd as pt
from padertorch_amd import _lib
from padertorch_amd.ops.losses import kl_divergence


def test_reachable_as_in_the_reference():
    fn = kl_divergence.gaussian_kl_divergence
    assert pt.ops.gaussian_kl_divergence is fn and pt.ops.losses.gaussian_kl_divergence is fn
    assert kl_divergence.__all__ == ['gaussian_kl_divergence']


def test_no_cpu_fallback():
    q = Normal(torch.zeros(3, 4), torch.ones(3, 4))
    for p in (Normal(torch.zeros(2, 4), torch.ones(2, 4)), MultivariateNormal(torch.zeros(2, 4), scale_tril=torch.eye(4).expand(2, 4, 4))):
        with pytest.raises(RuntimeError, match='no CPU fallback'):
            pt.ops.gaussian_kl_divergence(q, p)


def test_type_and_shape_checks():
    q, p = Normal(torch.zeros(3, 4), torch.ones(3, 4)), Normal(torch.zeros(2, 4), torch.ones(2, 4))
    with pytest.raises(AssertionError):
        pt.ops.gaussian_kl_divergence(MultivariateNormal(torch.zeros(3, 4), scale_tril=torch.eye(4)), p)
    with pytest.raises(ValueError):
        pt.ops.gaussian_kl_divergence(q, Laplace(torch.zeros(2, 4), torch.ones(2, 4)))
    with pytest.raises(AssertionError):
        pt.ops.gaussian_kl_divergence(q, Normal(torch.zeros(2, 5), torch.ones(2, 5)))


def test_limits_and_tiles():
    lib = _lib.load()
    assert lib.ptmi_gkl_max_features() == 64
    assert (lib.ptmi_gkl_row_tile(), lib.ptmi_gkl_split_rows()) == (kl_divergence.kGklBM, kl_divergence.kGklSplitRows)
    assert lib.ptmi_gkl_workspace_elems(2 * kl_divergence.kGklSplitRows + 3, 5, 20, 1) == 3 * 5 * (32 * 32 + 3 * 32)
    assert lib.ptmi_gkl_forward(None, None, None, None, None, None, 1, 4, 4, 65, None, None) == -2      # PTMI_E_UNSUPPORTED, no launch


def test_ops_have_a_cuda_kernel_only():
    for n in ('gkl_prepare', 'gkl_forward', 'gkl_backward'):
        assert torch._C._dispatch_has_kernel_for_dispatch_key(f'ptmi::{n}', 'CUDA')
        assert not torch._C._dispatch_has_kernel_for_dispatch_key(f'ptmi::{n}', 'CPU')
