"""The BigVGAN generator, inference only (reference: ``nvidia_bigvgan/bigvgan.py``): ``AMPBlock1``, ``AMPBlock2`` and ``BigVGAN`` with the
reference's constructor arguments, submodule and parameter names, so a reference ``state_dict`` - taken after ``remove_weight_norm()`` or
before it - loads with ``strict=True``.

Every activation is the fused :class:`~.alias_free_activation.Activation1d` launch; every convolution runs on the kernels of
``padertorch_amd/csrc/bigvgan.hip`` (:mod:`padertorch_amd.ops.bigvgan`).  The residual add of a block (``x = xt + x``) is the epilogue of
the convolution in front of it, and the mean over the parallel blocks of a stage is the epilogue of each block's last convolution, which
writes ``(xt + x) / num_kernels`` into the stage's one accumulator: neither is a launch of its own.

The weights are stored folded (``weight``, no ``weight_g`` / ``weight_v``): ``load_state_dict`` folds the weight-normed spellings
(``weight_g`` / ``weight_v`` and ``parametrizations.weight.original0`` / ``original1``) on the way in, and ``remove_weight_norm()`` has
nothing left to do.  Parameters are created with ``requires_grad=False``; there is no backward.  Checkpoints are read from a local
directory only (:meth:`BigVGAN.from_pretrained`): nothing here downloads.
"""
import json
from pathlib import Path

import torch
from torch import nn

from ......ops import bigvgan as ops
from .activations import Snake, SnakeBeta
from .alias_free_activation import Activation1d

__all__ = ['AttrDict', 'AMPBlock1', 'AMPBlock2', 'BigVGAN', 'load_hparams_from_json']


class AttrDict(dict):
    """A dict whose items are attributes too (the reference's ``env.AttrDict``)."""

    def __getattr__(self, name):
        try:
            return self[name]
        except KeyError:
            raise AttributeError(name) from None

    def __setattr__(self, name, value):
        self[name] = value


def load_hparams_from_json(path) -> AttrDict:
    return AttrDict(json.loads(Path(path).read_text()))


def _hparams(h):
    return h if isinstance(h, AttrDict) else AttrDict(h)


class _FoldedConv(nn.Module):
    """The parameters of a convolution the reference wraps in ``weight_norm``: ``weight`` (folded) and ``bias``."""

    def __init__(self, weight_shape, bias_size, bias=True):
        super().__init__()
        self.weight = nn.Parameter(torch.randn(weight_shape) * 0.01, requires_grad=False)      # init_weights: normal(0, 0.01)
        if bias:
            self.bias = nn.Parameter(torch.zeros(bias_size), requires_grad=False)
        else:
            self.register_parameter('bias', None)

    def _load_from_state_dict(self, state_dict, prefix, *args, **kwargs):
        for g, v in (('weight_g', 'weight_v'), ('parametrizations.weight.original0', 'parametrizations.weight.original1')):
            if prefix + g in state_dict and prefix + v in state_dict and prefix + 'weight' not in state_dict:
                state_dict[prefix + 'weight'] = ops.fold_weight_norm(state_dict.pop(prefix + g), state_dict.pop(prefix + v))
        super()._load_from_state_dict(state_dict, prefix, *args, **kwargs)


class _Conv1d(_FoldedConv):
    """``Conv1d(c_in, c_out, kernel_size, dilation=dilation, padding=(kernel_size - 1) dilation // 2)``."""

    def __init__(self, c_in, c_out, kernel_size, dilation=1, bias=True):
        super().__init__((c_out, c_in, kernel_size), c_out, bias)
        self.dilation = dilation

    def forward(self, x, **epilogue):
        return ops.conv1d(x, self.weight, self.bias, self.dilation, **epilogue)


class _ConvTranspose1d(_FoldedConv):
    """``ConvTranspose1d(c_in, c_out, kernel_size, stride, padding=(kernel_size - stride) // 2)``."""

    def __init__(self, c_in, c_out, kernel_size, stride):
        super().__init__((c_in, c_out, kernel_size), c_out)
        self.stride = stride

    def forward(self, x):
        return ops.conv_transpose1d(x, self.weight, self.bias, self.stride)


def _activations(h, channels, activation, count):
    if activation == 'snake':
        cls = Snake
    elif activation == 'snakebeta':
        cls = SnakeBeta
    else:
        raise NotImplementedError("activation incorrectly specified. check the config file and look for 'activation'.")
    return nn.ModuleList([Activation1d(activation=cls(channels, alpha_trainable=False, alpha_logscale=h.snake_logscale))
                          for _ in range(count)])


class AMPBlock1(nn.Module):
    """``x = c2(a2(c1(a1(x)))) + x`` per dilation (``convs2`` have dilation 1).  ``forward(x, out=None, scale=1.0, path=None)``: the last
    residual sum leaves as ``scale (xt + x)``, written to a new tensor or added to ``out`` - how :class:`BigVGAN` takes the mean over
    its blocks; ``path`` pins the convolutions' path (``ops.bigvgan.conv1d``)."""

    def __init__(self, h, channels: int, kernel_size: int = 3, dilation: tuple = (1, 3, 5), activation: str = None):
        super().__init__()
        self.h = h = _hparams(h)
        self.convs1 = nn.ModuleList([_Conv1d(channels, channels, kernel_size, d) for d in dilation])
        self.convs2 = nn.ModuleList([_Conv1d(channels, channels, kernel_size, 1) for _ in dilation])
        self.num_layers = len(self.convs1) + len(self.convs2)
        self.activations = _activations(h, channels, activation, self.num_layers)

    def forward(self, x, out=None, scale=1.0, path=None):
        acts1, acts2 = self.activations[::2], self.activations[1::2]
        last = len(self.convs1) - 1
        for i, (c1, c2, a1, a2) in enumerate(zip(self.convs1, self.convs2, acts1, acts2)):
            xt = c1(a1(x), path=path)
            xt = a2(xt)
            if i < last:
                x = c2(xt, residual=x, path=path)
            else:
                x = c2(xt, residual=x, out=out, accumulate=out is not None, scale=scale, path=path)
        return x

    def remove_weight_norm(self):
        pass


class AMPBlock2(nn.Module):
    """``x = c(a(x)) + x`` per dilation; ``forward`` as :class:`AMPBlock1`."""

    def __init__(self, h, channels: int, kernel_size: int = 3, dilation: tuple = (1, 3, 5), activation: str = None):
        super().__init__()
        self.h = h = _hparams(h)
        self.convs = nn.ModuleList([_Conv1d(channels, channels, kernel_size, d) for d in dilation])
        self.num_layers = len(self.convs)
        self.activations = _activations(h, channels, activation, self.num_layers)

    def forward(self, x, out=None, scale=1.0, path=None):
        last = len(self.convs) - 1
        for i, (c, a) in enumerate(zip(self.convs, self.activations)):
            if i < last:
                x = c(a(x), residual=x, path=path)
            else:
                x = c(a(x), residual=x, out=out, accumulate=out is not None, scale=scale, path=path)
        return x

    def remove_weight_norm(self):
        pass


class BigVGAN(nn.Module):
    """``forward(x [B, num_mels, T]) -> [B, 1, T prod(upsample_rates)]``.  ``h``: the hyper-parameters (an :class:`AttrDict` or any
    mapping); ``use_cuda_kernel`` is accepted for compatibility and ignored (every activation is the fused HIP launch), as ``fused=`` is
    on ``Activation1d``.  ``conv_path`` (``None``, ``'gemm'``, ``'direct'``) pins the path of every convolution: tests and measurements."""

    def __init__(self, h, use_cuda_kernel: bool = False):
        super().__init__()
        self.h = h = _hparams(h)
        self.h['use_cuda_kernel'] = use_cuda_kernel
        self.conv_path = None
        self.num_kernels = len(h.resblock_kernel_sizes)
        self.num_upsamples = len(h.upsample_rates)
        self.conv_pre = _Conv1d(h.num_mels, h.upsample_initial_channel, 7)
        if h.resblock == '1':
            resblock_class = AMPBlock1
        elif h.resblock == '2':
            resblock_class = AMPBlock2
        else:
            raise ValueError(f'Incorrect resblock class specified in hyperparameters. Got {h.resblock}')
        self.ups = nn.ModuleList()
        for i, (u, k) in enumerate(zip(h.upsample_rates, h.upsample_kernel_sizes)):
            self.ups.append(nn.ModuleList([_ConvTranspose1d(h.upsample_initial_channel // (2 ** i),
                                                            h.upsample_initial_channel // (2 ** (i + 1)), k, u)]))
        self.resblocks = nn.ModuleList()
        for i in range(len(self.ups)):
            ch = h.upsample_initial_channel // (2 ** (i + 1))
            for k, d in zip(h.resblock_kernel_sizes, h.resblock_dilation_sizes):
                self.resblocks.append(resblock_class(h, ch, k, d, activation=h.activation))
        self.activation_post = _activations(h, ch, h.activation, 1)[0]
        self.use_bias_at_final = h.get('use_bias_at_final', True)
        self.conv_post = _Conv1d(ch, 1, 7, bias=self.use_bias_at_final)
        self.use_tanh_at_final = h.get('use_tanh_at_final', True)

    def forward(self, x):
        path = self.conv_path
        x = self.conv_pre(x, path=path)
        for i in range(self.num_upsamples):
            for up in self.ups[i]:
                x = up(x)
            xs = None
            for j in range(self.num_kernels):
                # xs (+)= block(x) / num_kernels: the mean over the blocks, in the epilogue of each block's last convolution
                xs = self.resblocks[i * self.num_kernels + j](x, out=xs, scale=1.0 / self.num_kernels, path=path)
            x = xs
        x = self.activation_post(x)
        return ops.conv_post(x, self.conv_post.weight, self.conv_post.bias, tanh=self.use_tanh_at_final)

    def remove_weight_norm(self):
        """Nothing to do: the weights are stored folded (``load_state_dict`` folds ``weight_g`` / ``weight_v``)."""

    @classmethod
    def from_pretrained(cls, directory, map_location='cpu', use_cuda_kernel: bool = False):
        """The model of ``directory / config.json`` with the weights of ``directory / bigvgan_generator.pt`` (``{'generator':
        state_dict}``, as the reference saves it) - a local directory; nothing is downloaded."""
        directory = Path(directory)
        if not directory.is_dir():
            raise FileNotFoundError(f'{directory}: no such directory (BigVGAN checkpoints are read from a local directory: config.json '
                                    f'and bigvgan_generator.pt; padertorch_amd does not download them)')
        for name in ('config.json', 'bigvgan_generator.pt'):
            if not (directory / name).is_file():
                raise FileNotFoundError(f'{directory / name} is missing')
        model = cls(load_hparams_from_json(directory / 'config.json'), use_cuda_kernel=use_cuda_kernel)
        checkpoint = torch.load(directory / 'bigvgan_generator.pt', map_location=map_location, weights_only=True)
        model.load_state_dict(checkpoint['generator'])
        return model
