"""The transposed half of ``padertorch/contrib/je/modules/conv.py`` / ``conv_utils.py`` on the MI355X: ``ConvTranspose1d``,
``ConvTranspose2d``, ``CNNTranspose1d``, ``CNNTranspose2d``, ``Unpool1d``, ``Unpool2d`` and ``get_transpose_config``, with the reference's
constructor arguments, defaults, attributes, submodule names and return tuples.  ``conv`` / ``gate_conv`` are
``torch.nn.ConvTranspose1d`` / ``ConvTranspose2d`` and the norms this package's ``Normalization``, so a reference ``state_dict`` loads with
``strict=True``; the arithmetic is ``ops.je_conv_transpose`` (``csrc/je_conv_transpose.hip``): a phase-split direct
convolution that never touches an inserted zero.  The 1-D classes run on the same kernels as planes with one frequency row.

    ConvTranspose*.forward(x, sequence_lengths=None) -> (y, sequence_lengths)
    CNNTranspose*.forward(x, sequence_lengths=None, target_shape=None, target_sequence_lengths=None, pool_indices=None)
        -> (y, sequence_lengths[, pool_indices])
    Unpool*.forward(x, sequence_lengths=None, indices=None) -> (y, sequence_lengths)
    get_transpose_config(config) -> the mirrored config (CNN1d <-> CNNTranspose1d, CNN2d <-> CNNTranspose2d)

A quirk of the reference is kept: a transposed block normalises the UNTRIMMED convolution output with the already TRIMMED lengths and
trims afterwards, so the zeros behind a length land ``front`` positions early.  These names live in this module only (the package does
not re-export them).  Not built, as in ``conv.py``: ``state`` / ``return_state``, CUDA-resident lengths, a transposed hybrid.
"""
from collections import defaultdict
from copy import copy

import numpy as np
import torch
import torch.nn.functional as F
from torch import nn

from ....ops import je_conv as _ops
from ....ops import je_conv2d as _ops2
from ....ops import je_conv_transpose as _opst
from .conv import _CNN, CNN1d, _Conv, _norm_act, _norm_operands, _track
from .conv2d import CNN2d, _norm_act2d, _repeat
from .conv_utils import (LengthTable, Trim, _compute_transpose_out_size, activation_code, compute_conv_output_sequence_lengths,
                         compute_conv_output_shape, compute_pad_size, host_lengths, to_list, to_pair)

__all__ = ['ConvTranspose1d', 'ConvTranspose2d', 'CNNTranspose1d', 'CNNTranspose2d', 'Unpool1d', 'Unpool2d', 'get_transpose_config']


def _planes(x):
    """``x [B, C, T]`` or ``[B, C, F, T]`` as rows ``[B F T, C]`` and ``(B, F, T)``."""
    return _ops2.planes(x.unsqueeze(2) if x.dim() == 3 else x)


def _unplanes(r, B, F_, T, is_2d):
    y = _ops2.unplanes(r, B, F_, T)
    return y if is_2d else y.squeeze(2)


def _add(x, x_):
    a, B, F_, T = _planes(x)
    return _unplanes(_ops.add(a, _planes(x_)[0], B * F_, T), B, F_, T, x.dim() == 4)


class _Unpool(nn.Module):
    """Max unpooling where indices are given (``nn.MaxUnpool*`` on the padded plane, then the reference's trim), else nearest upsampling
    by the stride: ``forward(x, sequence_lengths=None, indices=None) -> (y, sequence_lengths)``."""
    def __init__(self, pool_size, stride=None, pad_type=None):
        super().__init__()
        self.pool_size = pool_size
        self.stride = pool_size if stride is None else stride
        self.pad_type = pad_type

    def forward(self, x, sequence_lengths=None, indices=None):
        # (the 1-D class: one row, a window of one on f)
        size, stride, pad = ([fill] * (2 - len(to_list(v))) + to_list(v) for v, fill in ((self.pool_size, 1), (self.stride, 1), (self.pad_type, None)))
        if all(k < 2 for k in size):
            return x, sequence_lengths
        r, B, F_in, T_in = _planes(x)
        if indices is None:
            front, out = (0, 0), (F_in * stride[0], T_in * stride[1])
        else:
            front = [compute_pad_size(k, 1, s, p)[0] for k, s, p in zip(size, stride, pad)]
            out = [int(_compute_transpose_out_size(n, k, 1, s, p)) for n, k, s, p in zip((F_in, T_in), size, stride, pad)]
            assert indices.shape == x.shape, (indices.shape, x.shape)
            indices = (indices.unsqueeze(2) if indices.dim() == 3 else indices).permute(0, 2, 3, 1).reshape(-1, x.shape[1])
        y = _opst.unpool(r, indices, [B, F_in, T_in, *out, x.shape[1], *size, *stride, *front])
        if sequence_lengths is not None:
            sequence_lengths = _compute_transpose_out_size(host_lengths(sequence_lengths), size[1], 1, stride[1], pad[1])
        return _unplanes(y, B, *out, x.dim() == 4), sequence_lengths


class Unpool1d(_Unpool):
    def __init__(self, pool_size, stride=None, pad_type=None):
        assert np.isscalar(pool_size)
        assert pad_type is None or np.isscalar(pad_type)
        super().__init__(pool_size, stride, pad_type)


class Unpool2d(_Unpool):
    def __init__(self, pool_size, stride=None, pad_type=None):
        super().__init__(to_pair(pool_size), None if stride is None else to_pair(stride), to_pair(pad_type))


class _ConvTranspose(_Conv):
    """``_Conv`` with ``torch.nn.ConvTranspose1d`` / ``2d`` inside: the shape and length functions with the ``transpose`` flag exchanged,
    and one fused block of ``ops.je_conv_transpose`` as ``forward``."""
    torch_cls = nn.ConvTranspose1d

    @classmethod
    def is_transpose(cls):
        return True

    @classmethod
    def is_2d(cls):
        return cls.torch_cls is nn.ConvTranspose2d

    def _axes(self):
        """``kernel_size, stride, dilation, pad_type`` as pairs ``(f, t)``; the 1-D block has one tap on ``f``."""
        if self.is_2d():
            return self.kernel_size, self.stride, self.dilation, self.pad_type
        return (1, self.kernel_size), (1, self.stride), (1, self.dilation), (None, self.pad_type)

    def forward(self, x, sequence_lengths=None, state=None, *, _table=None, _residual=None):
        if state is not None:
            raise NotImplementedError(f'{type(self).__name__}: state (the streaming mode) is not built')
        if self.training and self.dropout > 0.:
            x = F.dropout(x, self.dropout)
        r, B, F_in, T_in = _planes(x)
        lengths = host_lengths(sequence_lengths)
        out_lengths = None if lengths is None else self.get_output_sequence_lengths(lengths)
        kernel, stride, dilation, pad = self._axes()
        front, plane, full = [], [], []
        for n, k, s, d, p in zip((F_in, T_in), kernel, stride, dilation, pad):
            f, e = compute_pad_size(k, d, s, p)
            front.append(f)
            full.append((n - 1) * s + d * (k - 1) + 1)
            plane.append(full[-1] - f - max(e - s + 1, 0))
        # the reference normalises the untrimmed output (with the trimmed lengths) and trims afterwards: such a block writes the full plane
        untrimmed = self.norm is not None and not self.pre_activation and (full != plane)
        written, at = (full, (0, 0)) if untrimmed else (plane, tuple(front))
        norm_lengths = _repeat(lengths, F_in) if self.pre_activation else _repeat(out_lengths, written[0])
        table = LengthTable(x.device) if _table is None else _table
        code, p, slope = activation_code(self.activation_fn)
        kind, fixed = (None, None) if self.norm is None else _norm_operands(self.norm)
        cfg = _opst.TransposeConfig(B, F_in, T_in, *written, tuple(kernel), tuple(stride), tuple(dilation), at, kind,
                                    0. if self.norm is None else self.norm.eps, code, p, bool(self.pre_activation))
        res = None
        if _residual is not None and not untrimmed:
            res, *shape = _planes(_residual)
            assert (*shape, res.shape[1]) == (B, *plane, self.out_channels), (_residual.shape, B, plane)
        weights = [self.conv.weight, self.gate_conv.weight if self.gated else None]
        if not self.is_2d():
            weights = [None if w is None else w.unsqueeze(2) for w in weights]
        y, stats = _opst.conv_transpose_block(
            r, cfg, weights[0], self.conv.bias, weights[1], self.gate_conv.bias if self.gated else None,
            None if self.norm is None else self.norm.gamma, None if self.norm is None else self.norm.beta, slope, fixed,
            table.get(norm_lengths) if self.norm is not None else None, res)
        if self.norm is not None:
            _track(self.norm, stats)
        y = _ops2.unplanes(y, B, *written)
        if untrimmed:
            y = y[:, :, front[0]:front[0] + plane[0], front[1]:front[1] + plane[1]]
        y = y if self.is_2d() else y.squeeze(2)
        if _residual is not None and untrimmed:
            y = _add(y, _residual)
        return y, out_lengths

    def get_output_shape(self, input_shape):
        assert len(input_shape) == 3 + self.is_2d(), len(input_shape)
        assert input_shape[1] == self.in_channels, (input_shape[1], self.in_channels)
        return compute_conv_output_shape(input_shape, out_channels=self.out_channels, kernel_size=self.kernel_size, dilation=self.dilation,
                                         pad_type=self.pad_type, stride=self.stride, transpose=True)

    def get_input_shape(self, output_shape):
        assert len(output_shape) == 3 + self.is_2d(), len(output_shape)
        assert output_shape[1] == self.out_channels, (output_shape[1], self.out_channels)
        return compute_conv_output_shape(output_shape, out_channels=self.in_channels, kernel_size=self.kernel_size, dilation=self.dilation,
                                         pad_type=self.pad_type, stride=self.stride, transpose=False)

    def get_output_sequence_lengths(self, input_sequence_lengths, state=None):
        if state is not None:
            raise NotImplementedError(f'{type(self).__name__}: state (the streaming mode) is not built')
        input_sequence_lengths = np.array(input_sequence_lengths)
        assert input_sequence_lengths.ndim == 1, input_sequence_lengths.ndim
        return compute_conv_output_sequence_lengths(input_sequence_lengths, kernel_size=self.kernel_size, dilation=self.dilation,
                                                    stride=self.stride, pad_type=self.pad_type, transpose=True)

    def get_input_sequence_lengths(self, output_sequence_lengths):
        output_sequence_lengths = np.array(output_sequence_lengths)
        assert output_sequence_lengths.ndim == 1, output_sequence_lengths.ndim
        return compute_conv_output_sequence_lengths(output_sequence_lengths, kernel_size=self.kernel_size, dilation=self.dilation,
                                                    stride=self.stride, pad_type=self.pad_type, transpose=False)


class ConvTranspose1d(_ConvTranspose):
    torch_cls = nn.ConvTranspose1d


class ConvTranspose2d(_ConvTranspose):
    torch_cls = nn.ConvTranspose2d


def get_transpose_config(config, transpose_config=None):
    """The config of the mirrored stack (useful with autoencoders): channels, geometry lists and residual connections reversed, the
    factory exchanged for its counterpart.  Dense connections cannot be transposed."""
    mirror = {CNN1d: CNNTranspose1d, CNNTranspose1d: CNN1d, CNN2d: CNNTranspose2d, CNNTranspose2d: CNN2d}
    if config['factory'] not in mirror:
        raise ValueError(f'get_transpose_config: factory {config["factory"]} is none of {[c.__name__ for c in mirror]}')
    out = {} if transpose_config is None else transpose_config
    out['factory'] = mirror[config['factory']]
    channels = [config['in_channels']] + list(config['out_channels'])
    num_layers = len(config['out_channels'])
    if 'input_layer' in config:
        out['output_layer'] = config['input_layer']
    if 'output_layer' in config:
        out['input_layer'] = config['output_layer']
    if 'residual_connections' in config:
        out['residual_connections'] = None
        if config['residual_connections'] is not None:
            skips = defaultdict(list)
            for src_idx, destinations in enumerate(to_list(config['residual_connections'], num_layers)):
                for dst_idx in to_list(destinations):
                    if dst_idx is not None:
                        skips[num_layers - dst_idx].append(num_layers - src_idx)
            # (the reference's rule: a single source keeps a scalar destination)
            out['residual_connections'] = [None if i not in skips else skips[i][0] if len(skips) == 1 else sorted(skips[i])
                                           for i in range(num_layers)]
    if config.get('dense_connections') is not None:
        raise ValueError('dense connections cannot be transposed.')
    out['in_channels'] = channels[-1]
    out['out_channels'] = channels[:-1][::-1]
    for kw in ('kernel_size', 'pad_type', 'dilation', 'stride', 'pool_type', 'pool_size', 'pool_stride', 'norm'):
        if kw in config:
            out[kw] = config[kw][::-1] if isinstance(config[kw], list) else config[kw]
    for kw in ('activation_fn', 'pre_activation', 'dropout', 'gated', 'norm_kwargs'):
        if kw in config:
            out[kw] = config[kw]
    return out


class _CNNTranspose(_CNN):
    """The reference's ``_CNN`` with transposed blocks: unpooling in front of a layer, skip signals upsampled, and every layer trimmed
    to the shapes that lead to ``target_shape``."""
    conv_cls = ConvTranspose1d
    unpool_cls = Unpool1d
    _norm_act = staticmethod(_norm_act)
    _add = staticmethod(_add)

    @classmethod
    def is_transpose(cls):
        return True

    @classmethod
    def get_transpose_config(cls, config, transpose_config=None):
        assert config['factory'] == cls, (config['factory'], cls)
        return get_transpose_config(config, transpose_config)

    def forward(self, x, sequence_lengths=None, target_shape=None, target_sequence_lengths=None, pool_indices=None, state=None):
        assert x.dim() == 3 + self.is_2d(), (x.shape, self.is_2d())
        if state is not None:
            raise NotImplementedError(f'{type(self).__name__}: state (the streaming mode) is not built')
        sequence_lengths = host_lengths(sequence_lengths)
        output_shapes = output_sequence_lengths = None
        if target_shape is not None:
            expected, *output_shapes = self.get_shapes(target_shape=target_shape)
            assert (np.array(x.shape) == expected).all(), (x.shape, expected)
        if target_sequence_lengths is not None:
            expected, *output_sequence_lengths = self.get_sequence_lengths(target_sequence_lengths=host_lengths(target_sequence_lengths))
            assert sequence_lengths is not None and (sequence_lengths == np.array(expected)).all(), (sequence_lengths, expected)
        pool_indices = to_list(copy(pool_indices), self.num_layers)[::-1]
        table = LengthTable(x.device)
        skip_signals = []
        for i, conv in enumerate(self.convs):
            if any(np.array(to_list(self.pool_sizes[i])) > 1):
                x, sequence_lengths = self.unpool_cls(self.pool_sizes[i], self.pool_strides[i], self.pad_types[i])(
                    x, sequence_lengths, indices=pool_indices[i])
                for src_idx, x_ in enumerate(skip_signals):
                    if x_ is not None:
                        skip_signals[src_idx] = self.unpool_cls(self.pool_strides[i], pad_type=self.pad_types[i])(x_)[0]
            if i == 0 and self.input_norm is not None:
                x = self._norm_act(self.input_norm, self.input_activation_fn, x, sequence_lengths, table)
            skip_signals.append(x if self.residual_connections[i] + self.dense_connections[i] else None)
            # the skip signals follow this layer's stride and are cut to its output: none of that depends on the layer's output, so the
            # first residual connection that ends here is the block's own residual operand
            shape = [int(n) for n in conv.get_output_shape(x.shape)[2:]]
            if any(np.array(to_list(self.strides[i])) > 1):
                for src_idx, x_ in enumerate(skip_signals):
                    if x_ is not None:
                        skip_signals[src_idx] = self.unpool_cls(self.strides[i], pad_type=self.pad_types[i])(x_)[0]
            has_dense = any(x_ is not None and i + 1 in self.dense_connections[src] for src, x_ in enumerate(skip_signals))
            residuals = []
            for src_idx, x_ in enumerate(skip_signals):
                if x_ is not None and i + 1 in self.residual_connections[src_idx]:
                    size = np.array(x_.shape[2:]) - np.array(shape)
                    assert all(size >= 0), size
                    if any(size > 0):
                        assert output_shapes is not None
                        x_ = Trim(side='end')(x_, size=size)
                    if f'{src_idx}->{i + 1}' in self.residual_skip_convs:
                        x_, _ = self.residual_skip_convs[f'{src_idx}->{i + 1}'](x_, _table=table)
                    residuals.append(x_)
            fused = residuals.pop(0) if residuals and not has_dense else None
            x, sequence_lengths = conv(x, sequence_lengths=sequence_lengths, _table=table, _residual=fused)
            for src_idx, x_ in enumerate(skip_signals):
                if x_ is not None and i + 1 in self.dense_connections[src_idx]:
                    size = np.array(x_.shape[2:]) - np.array(x.shape[2:])
                    assert all(size >= 0), size
                    x = torch.cat((x, x_[(..., *[slice(0, n) for n in x.shape[2:]])]), dim=1)
            for x_ in residuals:
                x = self._add(x, x_)
            for src_idx in range(len(skip_signals)):
                destinations = self.dense_connections[src_idx] + self.residual_connections[src_idx]
                if destinations and max(destinations) <= i + 1:
                    skip_signals[src_idx] = None
            if i == self.num_layers - 1 and self.output_norm is not None:
                x = self._norm_act(self.output_norm, self.output_activation_fn, x, sequence_lengths, table)
            if output_shapes is not None:
                assert tuple(x.shape[:2]) == tuple(output_shapes[i])[:2], (x.shape, output_shapes[i])
                size = np.array(x.shape[2:]) - np.array(output_shapes[i][2:])
                assert all(size >= 0), (f'Desired output_shape {np.abs(size)} bins greater than actual output shape. '
                                        f'Maybe you did not use padding.')
                if any(size > 0):
                    x = Trim(side='end')(x, size=size)
            if output_sequence_lengths is not None:
                sequence_lengths = output_sequence_lengths[i]
        outputs = [x, sequence_lengths]
        if self.return_pool_indices:
            outputs.append(pool_indices)
        return tuple(outputs)

    def get_shapes(self, input_shape=None, target_shape=None):
        assert (input_shape is None) ^ (target_shape is None), (input_shape, target_shape)
        forward = input_shape is not None
        cur = input_shape if forward else target_shape
        shapes = [cur]
        layers = list(enumerate(self.convs))
        for i, conv in layers if forward else reversed(layers):
            if forward:
                cur = conv.get_output_shape(cur)
                cur[1] = self.layer_in_channels[i + 1]
            else:
                cur = np.copy(cur)
                cur[1] = conv.out_channels
                cur = conv.get_input_shape(cur)
            if self.pool_types[i] is not None:
                cur = compute_conv_output_shape(cur, out_channels=cur[1], kernel_size=self.pool_sizes[i], dilation=1,
                                                stride=self.pool_strides[i], pad_type=self.pad_types[i], transpose=forward)
            shapes.append(cur)
        return shapes if forward else shapes[::-1]

    def get_sequence_lengths(self, input_sequence_lengths=None, target_sequence_lengths=None):
        assert (input_sequence_lengths is None) ^ (target_sequence_lengths is None), (input_sequence_lengths, target_sequence_lengths)
        forward = input_sequence_lengths is not None
        cur = input_sequence_lengths if forward else target_sequence_lengths
        seq_lens = [cur]
        layers = list(enumerate(self.convs))
        for i, conv in layers if forward else reversed(layers):
            cur = conv.get_output_sequence_lengths(cur) if forward else conv.get_input_sequence_lengths(cur)
            if self.pool_types[i] is not None:
                cur = compute_conv_output_sequence_lengths(cur, kernel_size=self.pool_sizes[i], dilation=1, stride=self.pool_strides[i],
                                                           pad_type=self.pad_types[i], transpose=forward)
            seq_lens.append(cur)
        return seq_lens if forward else seq_lens[::-1]


class CNNTranspose1d(_CNNTranspose):
    conv_cls = ConvTranspose1d
    unpool_cls = Unpool1d


class CNNTranspose2d(_CNNTranspose):
    conv_cls = ConvTranspose2d
    unpool_cls = Unpool2d
    _norm_act = staticmethod(_norm_act2d)
