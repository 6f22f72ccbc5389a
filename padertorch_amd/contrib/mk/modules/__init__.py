"""``padertorch.contrib.mk.modules`` on the HIP path: ``contrastive`` (CPC1d on the fused InfoNCE kernels of ``csrc/cpc_contrast.hip``) and
``transformer`` (MultiheadAttention with RoPE, q/k RMS norm and the linear bias, the norms and the encoder on ``csrc/mk_attention.hip``)."""
from . import contrastive  # noqa: F401
from . import transformer  # noqa: F401
from .contrastive import CPC1d, CPCFeatureExtractor  # noqa: F401
