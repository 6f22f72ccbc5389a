from . import fully_connected, normalization, recurrent  # noqa: F401
from .fully_connected import fully_connected_stack  # noqa: F401
from .normalization import Normalization, InputNormalization, normalize  # noqa: F401
from .recurrent import StatefulLSTM  # noqa: F401
from . import convnet  # noqa: F401
from .convnet import ConvNet  # noqa: F401
from . import dual_path_rnn  # noqa: F401
from .dual_path_rnn import DPRNN, DPRNNBlock, _ChunkRNN, segment, overlap_add  # noqa: F401
from . import wavenet  # noqa: F401
from .wavenet import WaveNet  # noqa: F401
