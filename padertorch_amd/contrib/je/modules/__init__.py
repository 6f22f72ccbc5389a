from . import features  # noqa: F401
from . import transformer  # noqa: F401
from .transformer import MultiHeadAttention, TransformerLayer, TransformerLayerStack, get_causal_mask  # noqa: F401
