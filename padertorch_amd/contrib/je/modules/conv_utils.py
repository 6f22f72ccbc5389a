"""The helpers of ``padertorch/contrib/je/modules/conv_utils.py`` for the 1-D convolution stack: ``Pad``, ``Trim``, ``Pool1d``, ``to_pair``,
``to_list``, ``map_activation_fn``, ``compute_pad_size``, ``compute_conv_output_shape``, ``compute_conv_output_sequence_lengths`` and
``_finalize_norm_kwargs``, with the reference's arguments and results.

``Pool1d`` runs on the pool kernels of ``csrc/je_conv.hip`` (``ops.je_conv.pool``): its padding and the trailing trim are index
arithmetic there, the indices of max pooling count on the padded axis as ``nn.MaxPool1d(return_indices=True)`` gives them behind
``Pad`` / ``Trim``.  ``Pad`` (``mode='constant'`` only) and ``Trim`` are views / one ``F.pad``: the convolution blocks never call them.

Not built: ``Pool2d``, ``Unpool1d``, ``Unpool2d``.
"""
import math

import numpy as np
import torch
import torch.nn.functional as F
from torch import nn

from ....ops import je_conv as _ops

__all__ = ['Pad', 'Trim', 'Pool1d', 'to_pair', 'to_list', 'map_activation_fn', 'compute_pad_size', 'compute_conv_output_shape',
           'compute_conv_output_sequence_lengths']

#: the activations the kernels know: name -> module class
ACTIVATION_FN_MAP = {
    'identity': nn.Identity,
    'relu': nn.ReLU,
    'leaky_relu': nn.LeakyReLU,
    'elu': nn.ELU,
    'tanh': nn.Tanh,
    'sigmoid': nn.Sigmoid,
    'prelu': nn.PReLU,
}


def to_list(x, length=None):
    """``x`` as a list; a scalar (or string, or None) is repeated ``length`` times, a sequence must have that length."""
    if isinstance(x, (list, tuple)):
        x = list(x)
    elif isinstance(x, np.ndarray) and x.ndim > 0:
        x = x.tolist()
    else:
        x = [x] * (1 if length is None else length)
    if length is not None:
        assert len(x) == length, (len(x), length)
    return x


def to_pair(x):
    return tuple(to_list(x, 2))


def _split(side, size):
    """(front, end) of ``size`` positions on ``side``; 'both': the end takes the odd one."""
    if side is None or size < 1:
        assert size == 0, size
        return 0, 0
    if side == 'front':
        return size, 0
    if side == 'end':
        return 0, size
    if side == 'both':
        return size // 2, math.ceil(size / 2)
    raise ValueError(f'pad side {side} unknown')


class Pad(nn.Module):
    """Pads the time axis of ``x [B, C, T]`` by ``size`` zeros in front, at the end, or split between both."""
    def __init__(self, side='both', mode='constant'):
        super().__init__()
        self.side = side
        self.mode = mode

    def forward(self, x, size):
        assert x.dim() == 3, x.shape
        size, = to_list(size, 1)
        if not size:
            return x
        return F.pad(x, list(_split(self.side, int(size))), mode=self.mode)


class Trim(nn.Module):
    """The counterpart of ``Pad``: removes ``size`` positions of the time axis."""
    def __init__(self, side='both'):
        super().__init__()
        self.side = side

    def forward(self, x, size):
        assert x.dim() == 3, x.shape
        size, = to_list(size, 1)
        front, end = _split(self.side, int(size))
        return x[..., front:x.shape[-1] - end]


def compute_pad_size(kernel_size, dilation, stride, pad_type):
    """``(front, end)`` padding of a window of ``kernel_size`` taps ``dilation`` apart moved by ``stride``."""
    span = 1 + dilation * (kernel_size - 1)
    if pad_type is None:
        return 0, 0
    overlap, rest = max(span - stride, 0), min(stride - 1, span - 1)
    if pad_type == 'front':
        return overlap, rest
    if pad_type == 'both':
        return overlap // 2, rest + math.ceil(overlap / 2)
    if pad_type == 'end':
        return 0, span - 1
    raise ValueError(f'pad type {pad_type} unknown')


def _compute_conv_out_size(in_size, kernel_size, dilation, stride, pad_type):
    stride = kernel_size if stride is None else stride
    span = 1 + dilation * (kernel_size - 1)
    return 1 + (in_size + sum(compute_pad_size(kernel_size, dilation, stride, pad_type)) - span) // stride


def _compute_transpose_out_size(in_size, kernel_size, dilation, stride, pad_type):
    stride = kernel_size if stride is None else stride
    front, end = compute_pad_size(kernel_size, dilation, stride, pad_type)
    out = 1 + (in_size - 1) * stride + dilation * (kernel_size - 1)
    return np.asarray(out).astype(np.int64) - front - max(end - stride + 1, 0)


def compute_conv_output_shape(input_shape, out_channels, kernel_size, dilation, stride, pad_type, transpose=False):
    input_shape = np.array(input_shape)
    n = len(input_shape) - 2
    size = _compute_transpose_out_size if transpose else _compute_conv_out_size
    out = np.zeros_like(input_shape)
    out[0], out[1] = input_shape[0], out_channels
    for d, (k, dil, s, p) in enumerate(zip(to_list(kernel_size, n), to_list(dilation, n), to_list(stride, n), to_list(pad_type, n))):
        out[2 + d] = size(input_shape[2 + d], k, dil, s, p)
    assert all(out > 0), out
    return out.astype(np.int64)


def compute_conv_output_sequence_lengths(input_sequence_lengths, kernel_size, dilation, pad_type, stride, transpose=False):
    size = _compute_transpose_out_size if transpose else _compute_conv_out_size
    out = size(np.asarray(input_sequence_lengths), to_list(kernel_size)[-1], to_list(dilation)[-1], to_list(stride)[-1],
               to_list(pad_type)[-1])
    assert all(out > 0), out
    return out.astype(np.int64)


def _finalize_norm_kwargs(norm_kwargs, norm, num_channels, is_2d):
    fixed = ('data_format', 'shape', 'statistics_axis', 'batch_axis', 'sequence_axis')
    assert not any(k in norm_kwargs for k in fixed), norm_kwargs
    if is_2d:
        norm_kwargs = {'data_format': 'bcft', 'shape': (None, num_channels, None, None), **norm_kwargs}
    else:
        norm_kwargs = {'data_format': 'bct', 'shape': (None, num_channels, None), **norm_kwargs}
    if norm == 'batch':
        norm_kwargs['statistics_axis'] = 'btf' if is_2d else 'bt'
    elif norm == 'sequence':
        norm_kwargs['statistics_axis'] = 't'
    else:
        raise ValueError(f'{norm} normalization not known.')
    return norm_kwargs


def map_activation_fn(activation_fn):
    """The activation module of a name; only what the convolution kernels evaluate exists here, anything else raises."""
    if activation_fn in ('linear', None):
        activation_fn = 'identity'
    if isinstance(activation_fn, str):
        if activation_fn not in ACTIVATION_FN_MAP:
            raise NotImplementedError(f'activation_fn {activation_fn!r}: the convolution kernels evaluate {sorted(ACTIVATION_FN_MAP)}; there '
                                      f'is no library fallback')
        return ACTIVATION_FN_MAP[activation_fn]()
    if not callable(activation_fn):
        raise ValueError(f'Type {type(activation_fn)} not supported for activation_fn')
    activation_code(activation_fn)
    return activation_fn


def activation_code(fn):
    """``(kernel code, parameter, slope tensor or None)`` of an activation module."""
    codes = _ops.ACTIVATIONS
    if fn is None or type(fn) is nn.Identity:
        return codes['identity'], 0., None
    if type(fn) is nn.ReLU:
        return codes['relu'], 0., None
    if type(fn) is nn.LeakyReLU:
        return codes['leaky_relu'], float(fn.negative_slope), None
    if type(fn) is nn.ELU:
        return codes['elu'], float(fn.alpha), None
    if type(fn) is nn.Tanh:
        return codes['tanh'], 0., None
    if type(fn) is nn.Sigmoid:
        return codes['sigmoid'], 0., None
    if type(fn) is nn.PReLU:
        if fn.weight.numel() != 1:
            raise NotImplementedError('a PReLU with one parameter only: the kernels read one slope')
        return codes['prelu'], 0., fn.weight
    raise NotImplementedError(f'activation_fn {type(fn).__name__}: the convolution kernels evaluate {sorted(ACTIVATION_FN_MAP)}; there is '
                              f'no library fallback')


def host_lengths(sequence_lengths):
    """``sequence_lengths`` (list, numpy array or CPU tensor) as an int64 numpy vector; CUDA lengths are not built."""
    if sequence_lengths is None:
        return None
    if torch.is_tensor(sequence_lengths):
        if sequence_lengths.is_cuda:
            raise NotImplementedError('sequence_lengths on the GPU: the output lengths are host data as in the reference; pass a list, a '
                                      'numpy array or a CPU tensor')
        sequence_lengths = sequence_lengths.detach().numpy()
    out = np.asarray(sequence_lengths).astype(np.int64)
    assert out.ndim == 1, out.shape
    return out


class LengthTable:
    """The device copies of a call's length vectors: every vector given to :meth:`prepare` travels in ONE upload."""
    def __init__(self, device, vectors=()):
        self.device, self.rows = device, {}
        vectors = [v for v in vectors if v is not None]
        if vectors:
            from .... import _lib
            dev = _lib.host_to_device(np.stack(vectors), torch.int64, device)
            self.rows = {tuple(v.tolist()): dev[i] for i, v in enumerate(vectors)}

    def get(self, lengths):
        if lengths is None:
            return None
        key = tuple(int(n) for n in lengths)
        if key not in self.rows:
            from .... import _lib
            self.rows[key] = _lib.host_to_device(list(key), torch.int64, self.device)
        return self.rows[key]


def pool_geometry(T, pool_size, stride, pad_type):
    """``(front, T_out)`` of a pool over ``T`` positions: pad, trim the end to whole windows, count the windows."""
    front, end = compute_pad_size(pool_size, 1, stride, pad_type)
    padded = T + front + end
    if padded < pool_size:
        raise ValueError(f'Pool1d: {T} positions (padded: {padded}) are fewer than the pool size {pool_size}')
    padded -= (padded - pool_size) % stride
    return front, (padded - pool_size) // stride + 1


class Pool1d(nn.Module):
    """``nn.MaxPool1d`` / ``nn.AvgPool1d`` behind the reference's padding, on ``x [B, C, T]``:
    ``forward(x, sequence_lengths=None) -> (y, sequence_lengths, pool_indices)``."""
    def __init__(self, pool_type, pool_size, stride=None, pad_type=None):
        super().__init__()
        assert np.isscalar(pool_size)
        assert pad_type is None or np.isscalar(pad_type)
        self.pool_type = pool_type
        self.pool_size = pool_size
        self.stride = pool_size if stride is None else stride
        self.pad_type = pad_type

    def forward(self, x, sequence_lengths=None):
        if self.pool_size < 2:
            assert self.pool_size == 1, self.pool_size
            return x, sequence_lengths, None
        assert self.pool_type is not None, 'pool_size > 1 not allowed when pool_type is None'
        if self.pool_type not in ('max', 'avg'):
            raise ValueError(f'{self.pool_type} pooling unknown.')
        r, B, T = _ops.rows(x)
        front, T_out = pool_geometry(T, self.pool_size, self.stride, self.pad_type)
        y, index = _ops.pool(r, B, T, T_out, self.pool_size, self.stride, front, self.pool_type == 'max')
        if sequence_lengths is not None:
            sequence_lengths = _compute_conv_out_size(host_lengths(sequence_lengths), self.pool_size, 1, self.stride, self.pad_type)
            assert all(sequence_lengths > 0), sequence_lengths
        return _ops.unrows(y, B, T_out), sequence_lengths, None if index is None else _ops.unrows(index, B, T_out)
