"""``nvidia_bigvgan``: the BigVGAN generator for inference (:mod:`.bigvgan`: ``BigVGAN``, ``AMPBlock1``, ``AMPBlock2`` on the convolution
kernels of ``padertorch_amd/csrc/bigvgan.hip``) with its periodic activations and the alias-free resampling around them (the fused kernel
of ``padertorch_amd/csrc/anti_alias.hip``).  Training the generator, the discriminators, the checkpoint download and the mel front-end
are not part of this project."""
from .activations import Snake, SnakeBeta
from .alias_free_activation import Activation1d, DownSample1d, LowPassFilter1d, UpSample1d, kaiser_sinc_filter1d
from .bigvgan import AMPBlock1, AMPBlock2, AttrDict, BigVGAN

__all__ = ['Snake', 'SnakeBeta', 'Activation1d', 'UpSample1d', 'DownSample1d', 'LowPassFilter1d', 'kaiser_sinc_filter1d', 'BigVGAN',
           'AMPBlock1', 'AMPBlock2', 'AttrDict']
