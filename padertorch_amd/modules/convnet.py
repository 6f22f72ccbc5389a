"""The convolutional separator of Conv-TasNet (``padertorch/modules/convnet.py``: ``ConvNet``, ``_Conv1DBlock``, ``Conv1d``) on the
kernels of ``padertorch_amd.ops.tcn`` and the split-fp16 GEMM.

Inside the separator every activation is ``[B, T, C]`` with channels innermost: ``ConvNet.forward`` takes and returns ``(B, L, N)`` and
never transposes (the reference transposes at both ends, ``convnet.py:238-241``).  A block is

    input norm -> 1x1 conv (GEMM) -> [PReLU -> zero pad -> depthwise dilated conv -> PReLU, one kernel] -> norm -> 1x1 conv (GEMM) + x

The modules hold the reference's parameters under the reference's names (``state_dict`` keys, shapes and order; the input norm appears
as ``input_norm.*`` and ``input_conv.norm.*``, the second as ``norm.*`` and ``output_conv.norm.*``, because the reference registers the
same module twice), so a reference checkpoint loads with ``strict=True``; the torch convolutions themselves never run.
"""
from typing import Optional

import torch

from ..base import Module
from ..ops import tcn
from ..ops.mappings import ACTIVATION_FN_MAP

__all__ = ['ConvNet', 'Conv1d', 'GlobalChannelLayerNorm', 'TransposedLayerNorm', 'build_norm']


class GlobalChannelLayerNorm(torch.nn.Module):
    """gLN (``padertorch/contrib/jensheit/norm.py:34-70``): statistics per example over time and channels; ``beta`` / ``gamma``
    of shape ``(dim, 1)``.  ``forward(x [B, T, dim], stats=None)``."""
    groups = 'example'

    def __init__(self, dim, eps=1e-05):
        super().__init__()
        self.eps, self.normalized_dim = eps, dim
        self.beta = torch.nn.Parameter(torch.zeros(dim, 1))
        self.gamma = torch.nn.Parameter(torch.ones(dim, 1))

    def forward(self, x, stats=None):
        return tcn.channel_norm(x, self.gamma, self.beta, 'example', stats=stats, eps=self.eps)

    def extra_repr(self):
        return f'{self.normalized_dim}, eps={self.eps}'


class TransposedLayerNorm(torch.nn.LayerNorm):
    """cLN (``norm.py:10-32``): statistics per time step over the channels; ``weight`` / ``bias`` of shape ``(dim,)``.
    ``forward(x [B, T, dim])`` - the data is channel-last already, nothing is transposed."""
    groups = 'row'

    def __init__(self, normalized_shape, eps=1e-5):
        super().__init__(normalized_shape, eps, elementwise_affine=True)

    def forward(self, x, stats=None):
        return tcn.channel_norm(x, self.weight, self.bias, 'row', stats=None, eps=self.eps)


def build_norm(norm, dim):
    if norm not in ['cLN', 'gLN', 'BN']:
        raise RuntimeError(f'Unsupported normalize layer: {norm}')
    if norm == 'BN':
        raise NotImplementedError("norm='BN' (torch.nn.BatchNorm1d) has no HIP kernel here; use 'gLN' or 'cLN'")
    return TransposedLayerNorm(dim) if norm == 'cLN' else GlobalChannelLayerNorm(dim)


class Conv1d(Module):
    """Parameter holder of the reference's ``Conv1d`` (``convnet.py:17-111``): ``activation_fn``, ``norm`` (optional, shared) and
    ``conv`` (a ``torch.nn.Conv1d`` for its initialisation and ``state_dict``).  It does not compute on its own: ``_Conv1DBlock.forward``
    reads the parameters and runs the fused kernels."""

    def __init__(self, in_channels, out_channels, kernel_size, dropout=0., pad_type='both', groups=1, dilation=1, stride=1, bias=True,
                 norm=None, activation_fn='relu'):
        super().__init__()
        if dropout != 0. or stride != 1:
            raise NotImplementedError('Conv1d: dropout and stride are not used by the separator and have no kernel here')
        self.in_channels, self.out_channels, self.bias, self.dropout = in_channels, out_channels, bias, dropout
        self.pad_type, self.kernel_size, self.dilation, self.stride = pad_type, kernel_size, dilation, stride
        self.activation_fn = ACTIVATION_FN_MAP[activation_fn]()
        if norm is not None:
            assert callable(norm), norm
        self.norm = norm
        self.conv = torch.nn.Conv1d(in_channels, out_channels, kernel_size=kernel_size, dilation=dilation, stride=stride, bias=bias,
                                    groups=groups)

    def forward(self, x):
        raise NotImplementedError('Conv1d holds parameters only; call the _Conv1DBlock it belongs to')


class _Conv1DBlock(Module):
    """norm - 1x1 conv - PReLU - depthwise dilated conv - PReLU - norm - 1x1 conv, plus the input (``convnet.py:114-161``);
    ``x [B, T, in_channels]`` -> the same shape."""

    def __init__(self, in_channels=256, hidden_channels=512, kernel_size=3, dilation=1, norm='cLN'):
        super().__init__()
        self.input_norm = build_norm(norm, in_channels)
        self.input_conv = Conv1d(in_channels, hidden_channels, 1, pad_type=None, norm=self.input_norm, activation_fn='prelu')
        self.conv = Conv1d(hidden_channels, hidden_channels, kernel_size, groups=hidden_channels, activation_fn='prelu', pad_type='both',
                           dilation=dilation)
        self.norm = build_norm(norm, hidden_channels)
        self.output_conv = Conv1d(hidden_channels, in_channels, 1, norm=self.norm, activation_fn='identity')

    def forward(self, x):
        u = tcn.pointwise_conv(self.input_norm(x), self.input_conv.conv.weight, self.input_conv.conv.bias)
        v, stats = tcn.depthwise_prelu(u, self.input_conv.activation_fn.weight, self.conv.conv.weight, self.conv.conv.bias,
                                       self.conv.activation_fn.weight, self.conv.dilation, self.conv.kernel_size, eps=self.norm.eps)
        y = self.norm(v, stats if self.norm.groups == 'example' else None)
        return tcn.pointwise_conv(y, self.output_conv.conv.weight, self.output_conv.conv.bias, residual=x)


class ConvNet(Module):
    """Convolutional separator of Conv-TasNet (https://arxiv.org/abs/1809.07454), ``padertorch/modules/convnet.py:164-241``:
    ``num_repeats`` stacks of ``num_blocks`` blocks with dilations ``1 .. 2 ** (num_blocks - 1)``.

    ``forward(sequence (B, L, N), sequence_lengths=None) -> (B, L, N)``.  ``sequence_lengths`` is accepted and IGNORED, exactly as in the
    reference: padded frames take part in the convolutions and in the gLN statistics."""

    def __init__(self, input_size=256, num_blocks=8, num_repeats=4, hidden_channels=512, kernel_size=3, norm='gLN'):
        super().__init__()
        self.input_size = input_size
        self.hidden_size = input_size
        self.conv_blocks = torch.nn.Sequential(*[
            torch.nn.Sequential(*[
                _Conv1DBlock(in_channels=input_size, hidden_channels=hidden_channels, kernel_size=kernel_size, norm=norm,
                             dilation=2 ** b)
                for b in range(num_blocks)])
            for _ in range(num_repeats)])

    def forward(self, sequence: torch.Tensor, sequence_lengths: Optional[torch.Tensor] = None) -> torch.Tensor:
        if sequence.dim() != 3 or sequence.shape[2] != self.input_size:
            raise ValueError(f'ConvNet: sequence (B, L, {self.input_size}), got {tuple(sequence.shape)}')
        return self.conv_blocks(sequence)
