"""``padertorch.contrib.mk.modules`` on the HIP path: ``contrastive`` (CPC1d on the fused InfoNCE kernels of ``csrc/cpc_contrast.hip``)."""
from . import contrastive  # noqa: F401
from .contrastive import CPC1d, CPCFeatureExtractor  # noqa: F401
