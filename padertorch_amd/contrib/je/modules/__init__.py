from . import features  # noqa: F401
from . import transformer  # noqa: F401
from .transformer import MultiHeadAttention, TransformerLayer, TransformerLayerStack, get_causal_mask  # noqa: F401
from . import reduce  # noqa: F401
from . import rnn  # noqa: F401
from .reduce import AutoPool, Max, Mean, Sum, TakeLast  # noqa: F401
from .rnn import GRU, LSTM, RNN, TransformerEncoder, reverse_sequence  # noqa: F401
