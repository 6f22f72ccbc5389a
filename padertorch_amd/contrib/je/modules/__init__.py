from . import features  # noqa: F401
from . import transformer  # noqa: F401
from .transformer import MultiHeadAttention, TransformerLayer, TransformerLayerStack, get_causal_mask  # noqa: F401
from . import reduce  # noqa: F401
from . import rnn  # noqa: F401
from . import conv  # noqa: F401
from . import conv_utils  # noqa: F401
from .conv import CNN1d, Conv1d  # noqa: F401
from .conv_utils import (Pad, Pool1d, Trim, compute_conv_output_sequence_lengths, compute_conv_output_shape,  # noqa: F401
                         compute_pad_size, map_activation_fn, to_list, to_pair)
from .reduce import AutoPool, Max, Mean, Sum, TakeLast  # noqa: F401
from .rnn import GRU, LSTM, RNN, TransformerEncoder, reverse_sequence  # noqa: F401
