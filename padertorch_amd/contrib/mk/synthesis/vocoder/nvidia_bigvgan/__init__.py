"""``nvidia_bigvgan``: the periodic activations and the alias-free resampling around them, on the fused HIP kernel of
``padertorch_amd/csrc/anti_alias.hip``.  The generator, its checkpoint download and the mel front-end are not part of this project."""
from .activations import Snake, SnakeBeta
from .alias_free_activation import Activation1d, DownSample1d, LowPassFilter1d, UpSample1d, kaiser_sinc_filter1d

__all__ = ['Snake', 'SnakeBeta', 'Activation1d', 'UpSample1d', 'DownSample1d', 'LowPassFilter1d', 'kaiser_sinc_filter1d']
