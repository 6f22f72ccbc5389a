"""mu-law companding on the HIP kernels of ``csrc/wavenet.hip`` (reference: ``padertorch/ops/mu_law.py``).

    mu_law_encode(x, mu_quantization=256, check=True)    float signal in [-1, 1] -> int64 codes in [0, mu_quantization - 1]
    mu_law_decode(x, mu_quantization=256, check=True)    codes -> float32 signal

The reference's range assertions are host reads: they stay on by default, ``check=False`` skips them.  The kernels clamp the codes to
``[0, mu_quantization - 1]`` either way and evaluate the logarithm / power in fp64 per element.  GPU tensors only.
"""
import torch

from .. import _lib
from . import library  # noqa: F401  (registers torch.ops.ptmi.mu_law_*)

__all__ = ['mu_law_encode', 'mu_law_decode']


def mu_law_decode(x, mu_quantization=256, check=True):
    _lib.require_gpu(x)
    if check and x.numel():
        assert torch.max(x) <= mu_quantization - 1
        assert torch.min(x) >= 0
    if x.dtype != torch.int64:
        x = x.to(torch.float32) if x.is_floating_point() else x.to(torch.int64)
    return torch.ops.ptmi.mu_law_decode(x.contiguous(), int(mu_quantization))


def mu_law_encode(x, mu_quantization=256, check=True):
    _lib.require_gpu(x)
    if x.dtype != torch.float32:
        raise NotImplementedError(f'mu_law_encode: float32 only, got {x.dtype}')
    if check and x.numel():
        assert torch.max(x) <= 1.0
        assert torch.min(x) >= -1.0
    return torch.ops.ptmi.mu_law_encode(x.contiguous(), int(mu_quantization))
