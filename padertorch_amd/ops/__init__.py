from .losses import *  # noqa: F401,F403
from . import losses
from . import sequence
from . import mappings
from . import scalars  # noqa: F401

from ._stft import STFT  # noqa: F401
from .einsum import *  # noqa: F401,F403
from .sequence import *  # noqa: F401,F403
from .features import pit_features  # noqa: F401
from . import gemm  # noqa: F401
from . import lstm  # noqa: F401
from . import linear  # noqa: F401
from .lstm import packed_lstm  # noqa: F401
from .unit_norm import unit_norm  # noqa: F401
from . import tas  # noqa: F401
from .tas import tas_encode, tas_decode, tas_masked_decode  # noqa: F401
from . import stft_coders  # noqa: F401
from .stft_coders import stft_encode, istft_decode, istft_masked_decode  # noqa: F401
from . import tcn  # noqa: F401
from .tcn import depthwise_prelu, channel_norm  # noqa: F401
from . import tasnet  # noqa: F401
from . import orpit  # noqa: F401
from . import dprnn  # noqa: F401
from . import beamforming  # noqa: F401
from .beamforming import (get_power_spectral_density_matrix, get_mvdr_vector_souden, apply_beamforming_vector,  # noqa: F401
                          mask_beamforming, get_gev_vector, get_pca_vector, blind_analytic_normalization, phase_correction,
                          get_bf_vector)
from . import mask_loss  # noqa: F401
from .mask_loss import mask_bce_loss  # noqa: F401
from . import griffin_lim  # noqa: F401
from .griffin_lim import gl_project, gl_update, gl_iterations  # noqa: F401
from . import anti_alias  # noqa: F401
from .anti_alias import anti_alias_activation, kaiser_sinc_filter1d  # noqa: F401
from . import mu_law  # noqa: F401
from .mu_law import mu_law_encode, mu_law_decode  # noqa: F401
from . import wavenet  # noqa: F401
from . import bigvgan  # noqa: F401
from . import attention  # noqa: F401
from .attention import scaled_dot_product_attention  # noqa: F401
from . import gru  # noqa: F401
from .gru import chunk_gru  # noqa: F401
from . import seq_pool  # noqa: F401
from .seq_pool import reverse_sequence  # noqa: F401
from . import je_conv  # noqa: F401
