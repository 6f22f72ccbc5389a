"""The alias-free activation of BigVGAN (reference: ``alias_free_activation/torch/{filter,resample,act}.py`` and the ``fused=`` keyword of
``alias_free_activation/cuda/activation1d.py``): constructors, attribute and buffer names of the reference, so its checkpoints load; the
filters in the buffers are the ones the kernel applies.

``Activation1d`` around a :class:`~..activations.Snake` / ``SnakeBeta`` is ONE launch (up-sampling, activation, low-pass and decimation,
the up-sampled signal never leaves the chip), forward and backward.  Around any other module it is the up-sampling launch, the module,
the down-sampling launch."""
from torch import nn

from .......ops import anti_alias
from .......ops.anti_alias import kaiser_sinc_filter1d
from ..activations import Snake, SnakeBeta

__all__ = ['kaiser_sinc_filter1d', 'LowPassFilter1d', 'UpSample1d', 'DownSample1d', 'Activation1d']


class LowPassFilter1d(nn.Module):
    def __init__(self, cutoff=0.5, half_width=0.6, stride: int = 1, padding: bool = True, padding_mode: str = 'replicate',
                 kernel_size: int = 12):
        super().__init__()
        if not 0 <= cutoff <= 0.5:
            raise ValueError(f'LowPassFilter1d: cutoff {cutoff!r} is outside [0, 0.5] (in units of the sampling rate)')
        if padding_mode != 'replicate':
            raise NotImplementedError(f'LowPassFilter1d: the HIP kernel pads by replication only, not {padding_mode!r}')
        anti_alias.check_stage(stride, kernel_size, up=False)
        self.kernel_size = kernel_size
        self.even = kernel_size % 2 == 0
        self.pad_left = kernel_size // 2 - int(self.even)
        self.pad_right = kernel_size // 2
        self.stride = stride
        self.padding = padding
        self.padding_mode = padding_mode
        self.register_buffer('filter', kaiser_sinc_filter1d(cutoff, half_width, kernel_size))

    def forward(self, x):
        return anti_alias.lowpass1d(x, self.filter, self.stride, self.padding)


class UpSample1d(nn.Module):
    def __init__(self, ratio=2, kernel_size=None):
        super().__init__()
        self.ratio = ratio
        self.kernel_size = anti_alias.default_kernel_size(ratio) if kernel_size is None else kernel_size
        anti_alias.check_stage(self.ratio, self.kernel_size, up=True)
        self.stride = ratio
        self.pad = self.kernel_size // ratio - 1
        self.pad_left = self.pad * self.stride + (self.kernel_size - self.stride) // 2
        self.pad_right = self.pad * self.stride + (self.kernel_size - self.stride + 1) // 2
        self.register_buffer('filter', kaiser_sinc_filter1d(cutoff=0.5 / ratio, half_width=0.6 / ratio, kernel_size=self.kernel_size))

    def forward(self, x):
        return anti_alias.upsample1d(x, self.filter, self.ratio)


class DownSample1d(nn.Module):
    def __init__(self, ratio=2, kernel_size=None):
        super().__init__()
        self.ratio = ratio
        self.kernel_size = anti_alias.default_kernel_size(ratio) if kernel_size is None else kernel_size
        self.lowpass = LowPassFilter1d(cutoff=0.5 / ratio, half_width=0.6 / ratio, stride=ratio, kernel_size=self.kernel_size)

    def forward(self, x):
        return self.lowpass(x)


class Activation1d(nn.Module):
    """``fused`` is accepted for compatibility with the reference's CUDA variant; both values run the HIP path."""

    def __init__(self, activation, up_ratio: int = 2, down_ratio: int = 2, up_kernel_size: int = 12, down_kernel_size: int = 12,
                 fused: bool = True):
        super().__init__()
        self.up_ratio = up_ratio
        self.down_ratio = down_ratio
        self.act = activation
        self.upsample = UpSample1d(up_ratio, up_kernel_size)
        self.downsample = DownSample1d(down_ratio, down_kernel_size)
        self.fused = fused

    def forward(self, x):
        if isinstance(self.act, (Snake, SnakeBeta)):
            alpha, beta = self.act.kernel_parameters()
            return anti_alias.anti_alias_activation(x, alpha, beta, up_filter=self.upsample.filter, down_filter=self.downsample.lowpass.filter,
                                                    up_ratio=self.up_ratio, down_ratio=self.down_ratio,
                                                    alpha_logscale=self.act.alpha_logscale)
        return self.downsample(self.act(self.upsample(x)))
