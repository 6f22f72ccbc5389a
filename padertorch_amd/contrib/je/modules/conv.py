"""``Conv1d`` and ``CNN1d`` of ``padertorch/contrib/je/modules/conv.py`` on the MI355X, with the reference's constructor arguments, defaults,
attributes, submodule names and return tuples.  ``conv`` and ``gate_conv`` are ``torch.nn.Conv1d``, ``norm`` / ``input_norm`` /
``output_norm`` this package's ``modules.normalization.Normalization``: the parameters and buffers are those modules' own, so a reference
``state_dict`` loads with ``strict=True``; only the arithmetic moves to ``ops.je_conv`` (``csrc/je_conv.hip``).

    Conv1d.forward(x [B, C, T], sequence_lengths=None) -> (y, sequence_lengths)
    CNN1d.forward(x, sequence_lengths=None) -> (y, sequence_lengths[, pool_indices])

Inside, an activation is held as channels-last rows ``[B T, C]``: a contiguous ``[B, C, T]`` input is brought there by one gather launch,
a layer returns the transposed VIEW of its rows, and the next layer reads that view in place.  Lengths come in as a list, numpy array or
CPU tensor and go out as an int64 numpy array; a call uploads them once.  The convolution does not mask: it reads and writes behind the
lengths as the reference does; only the normalisation masks (statistics over ``t < len_b``, zero output behind).  ``dropout > 0`` in
training calls ``F.dropout``, a library kernel - the one exception.  Activations: identity / linear / None, relu, leaky_relu, elu, tanh,
sigmoid, prelu (one parameter).  ``Conv1d.forward`` has two keyword-only arguments the reference does not, ``_table`` and ``_residual``:
they are private, the route by which a ``CNN1d`` hands its one length upload and the fused residual operand to its layers.

A departure: non-finite values BEHIND a length invalidate the call.  They stay out of the statistics' sums and the output behind the
length is zero, as in the reference, but the layer's channel product is a planes GEMM whose operand scale is the maximum over ALL rows
(``ops.gemm`` takes a non-finite maximum as the largest finite float), so one NaN or infinity in the padding spoils every row of that
GEMM's output in front of the lengths too - and with it the statistics computed from it.  The reference confines such a value to the
positions whose window holds it.  Pad with finite values (zeros), as every layer here does for the next.

Not built (``NotImplementedError``, no library fallback): ``state`` / ``return_state`` (the streaming mode), CUDA-resident
``sequence_lengths``, ``get_transpose_config``, other activations or callables, a normalisation with ``shift=False`` or ``scale=False``, and
the transposed and 2-D classes (``ConvTranspose1d``, ``Conv2d``, ``ConvTranspose2d``, ``CNNTranspose1d``, ``CNN2d``, ``CNNTranspose2d``,
``Pool2d``, ``Unpool1d``, ``Unpool2d``, ``resnet50``, ``hybrid.py``), which are not defined here at all.
"""
from copy import copy
from typing import List

import numpy as np
import torch
import torch.nn.functional as F
from torch import nn

from ....modules.normalization import Normalization
from ....ops import je_conv as _ops
from .conv_utils import (LengthTable, Pool1d, _finalize_norm_kwargs, activation_code, compute_conv_output_sequence_lengths,
                         compute_conv_output_shape, compute_pad_size, host_lengths, map_activation_fn, to_list)

__all__ = ['Conv1d', 'CNN1d']


def _norm_operands(norm):
    """``(kind, fixed statistics or None)`` of a ``Normalization`` for the kernels."""
    if not (norm.shift and norm.scale):
        raise NotImplementedError('a Normalization with shift=False or scale=False is not built: the convolution kernels centre and scale')
    kind = 'batch' if norm.track_running_stats else 'sequence'
    if not norm.track_running_stats or (norm.training and not norm.frozen_stats):
        return kind, None
    with torch.no_grad():
        mean = norm.running_mean.reshape(-1)
        rstd = torch.rsqrt(norm.running_var.reshape(-1) + norm.eps)           # eps enters twice, as in Normalization._running_norm
        return kind, torch.stack([mean, rstd, rstd, rstd]).unsqueeze(0).contiguous()


def _track(norm, stats):
    """The running buffers of ``norm`` from the statistics ``[1, 4, C]`` the kernels measured."""
    if stats is not None and norm.track_running_stats:
        shape = norm.running_mean.shape
        with torch.no_grad():
            norm._update_running_stats(stats[0, 0].view(shape), stats[0, 2].view(shape), stats[0, 3].view(shape))


def _norm_act(norm, activation_fn, x, lengths, table):
    """``activation_fn(norm(x))`` on ``x [B, C, T]`` (``input_norm`` / ``output_norm``)."""
    r, B, T = _ops.rows(x)
    code, p, slope = activation_code(activation_fn)
    kind, fixed = _norm_operands(norm)
    out, stats = _ops.norm_act(r, B, T, kind, norm.eps, code, p, norm.gamma, norm.beta, slope, fixed, table.get(lengths))
    _track(norm, stats)
    return _ops.unrows(out, B, T)


class Conv1d(nn.Module):
    """``torch.nn.Conv1d`` with padding, an optional gate convolution, normalisation and activation of its output (or, ``pre_activation``,
    of its input) - one fused block of ``ops.je_conv``."""

    def __init__(self, in_channels, out_channels, kernel_size, dropout=0., pad_type='both', dilation=1, stride=1, bias=True, norm=None,
                 norm_kwargs=None, activation_fn='relu', pre_activation=False, gated=False, return_state=False):
        super().__init__()
        if return_state:
            raise NotImplementedError('Conv1d: return_state (the streaming mode) is not built')
        self.in_channels = in_channels
        self.out_channels = out_channels
        self.bias = bias
        self.dropout = dropout
        self.pad_type = pad_type
        self.kernel_size = kernel_size
        self.dilation = dilation
        self.stride = stride
        self.activation_fn = map_activation_fn(activation_fn)
        self.pre_activation = pre_activation
        self.gated = gated
        self.return_state = return_state
        self.conv = nn.Conv1d(in_channels, out_channels, kernel_size=kernel_size, dilation=dilation, stride=stride, bias=bias)
        if self.gated:
            self.gate_conv = nn.Conv1d(in_channels, out_channels, kernel_size=kernel_size, dilation=dilation, stride=stride, bias=bias)
        if norm is None:
            self.norm = None
            assert norm_kwargs is None, norm_kwargs
        else:
            num_channels = self.in_channels if self.pre_activation else self.out_channels
            self.norm = Normalization(**_finalize_norm_kwargs({} if norm_kwargs is None else norm_kwargs, norm, num_channels, False))
            _norm_operands(self.norm)                           # (refuses shift=False / scale=False here, not in the first call)

    @classmethod
    def is_transpose(cls):
        return False

    @classmethod
    def is_2d(cls):
        return False

    def reset_parameters(self, output_activation_fn):
        if isinstance(self.activation_fn, nn.PReLU):
            with torch.no_grad():
                self.activation_fn.weight.fill_(.25)
        output_activation_fn = map_activation_fn(output_activation_fn)
        if isinstance(output_activation_fn, (nn.ReLU, nn.ELU)):
            nn.init.kaiming_uniform_(self.conv.weight, nonlinearity='relu')
        elif isinstance(output_activation_fn, nn.LeakyReLU):
            nn.init.kaiming_uniform_(self.conv.weight, nonlinearity='leaky_relu', a=output_activation_fn.negative_slope)
        elif isinstance(output_activation_fn, nn.PReLU):
            nn.init.kaiming_uniform_(self.conv.weight, nonlinearity='leaky_relu', a=.25)
        else:
            nn.init.xavier_uniform_(self.conv.weight, gain=5 / 3 if isinstance(output_activation_fn, nn.Tanh) else 1.)
        if self.gated:
            nn.init.xavier_uniform_(self.gate_conv.weight, gain=1.)
        if self.bias:
            nn.init.zeros_(self.conv.bias)
            if self.gated:
                nn.init.zeros_(self.gate_conv.bias)

    def freeze(self, freeze_norm_stats=True):
        for param in self.parameters():
            param.requires_grad = False
        if self.norm is not None:
            self.norm.freeze(freeze_stats=freeze_norm_stats)

    def forward(self, x, sequence_lengths=None, state=None, *, _table=None, _residual=None):
        if state is not None:
            raise NotImplementedError('Conv1d: state (the streaming mode) is not built')
        if self.training and self.dropout > 0.:
            x = F.dropout(x, self.dropout)
        r, B, T = _ops.rows(x)
        lengths = host_lengths(sequence_lengths)
        out_lengths = None if lengths is None else self.get_output_sequence_lengths(lengths)
        table = LengthTable(x.device, [lengths, out_lengths]) if _table is None else _table
        T_out = int(self.get_output_shape((B, self.in_channels, T))[2])
        front, _ = compute_pad_size(self.kernel_size, self.dilation, self.stride, self.pad_type)
        code, p, slope = activation_code(self.activation_fn)
        kind, fixed = (None, None) if self.norm is None else _norm_operands(self.norm)
        cfg = _ops.BlockConfig(B, T, T_out, self.kernel_size, self.stride, self.dilation, front, kind,
                               0. if self.norm is None else self.norm.eps, code, p, bool(self.pre_activation))
        res = None
        if _residual is not None:
            res, rb, rt = _ops.rows(_residual)
            assert (rb, rt, res.shape[1]) == (B, T_out, self.out_channels), (_residual.shape, B, T_out)
        y, stats = _ops.conv_block(
            r, cfg, self.conv.weight, self.conv.bias, self.gate_conv.weight if self.gated else None,
            self.gate_conv.bias if self.gated else None, None if self.norm is None else self.norm.gamma,
            None if self.norm is None else self.norm.beta, slope, fixed,
            table.get(lengths if self.pre_activation else out_lengths) if self.norm is not None else None, res)
        if self.norm is not None:
            _track(self.norm, stats)
        return _ops.unrows(y, B, T_out), out_lengths

    def get_output_shape(self, input_shape):
        assert len(input_shape) == 3, len(input_shape)
        assert input_shape[1] == self.in_channels, (input_shape[1], self.in_channels)
        return compute_conv_output_shape(input_shape, out_channels=self.out_channels, kernel_size=self.kernel_size, dilation=self.dilation,
                                         pad_type=self.pad_type, stride=self.stride, transpose=False)

    def get_input_shape(self, output_shape):
        assert len(output_shape) == 3, len(output_shape)
        assert output_shape[1] == self.out_channels, (output_shape[1], self.out_channels)
        return compute_conv_output_shape(output_shape, out_channels=self.in_channels, kernel_size=self.kernel_size, dilation=self.dilation,
                                         pad_type=self.pad_type, stride=self.stride, transpose=True)

    def get_output_sequence_lengths(self, input_sequence_lengths, state=None):
        if state is not None:
            raise NotImplementedError('Conv1d: state (the streaming mode) is not built')
        input_sequence_lengths = np.array(input_sequence_lengths)
        assert input_sequence_lengths.ndim == 1, input_sequence_lengths.ndim
        return compute_conv_output_sequence_lengths(input_sequence_lengths, kernel_size=self.kernel_size, dilation=self.dilation,
                                                    stride=self.stride, pad_type=self.pad_type, transpose=False)

    def get_input_sequence_lengths(self, output_sequence_lengths):
        output_sequence_lengths = np.array(output_sequence_lengths)
        assert output_sequence_lengths.ndim == 1, output_sequence_lengths.ndim
        return compute_conv_output_sequence_lengths(output_sequence_lengths, kernel_size=self.kernel_size, dilation=self.dilation,
                                                    stride=self.stride, pad_type=self.pad_type, transpose=True)


class CNN1d(nn.Module):
    """A stack of ``Conv1d`` blocks with residual and dense connections and pooling (the reference's ``CNN1d``)."""
    conv_cls = Conv1d

    def __init__(self, in_channels, out_channels: List[int], kernel_size, input_layer=True, output_layer=True, residual_connections=None,
                 dense_connections=None, dropout=0., pad_type='both', dilation=1, stride=1, norm=None, norm_kwargs=None,
                 activation_fn='relu', pre_activation=False, gated=False, pool_type='max', pool_size=1, pool_stride=None,
                 return_pool_indices=False, return_state=False, normalize_skip_convs=False):
        super().__init__()
        if return_state:
            raise NotImplementedError('CNN1d: return_state (the streaming mode) is not built')
        self.in_channels = in_channels
        self.out_channels = copy(out_channels)
        num_layers = len(out_channels)
        self.num_layers = num_layers
        self.kernel_sizes = to_list(kernel_size, num_layers)
        self.residual_connections = [[] if dst is None else to_list(dst) for dst in to_list(residual_connections, num_layers)]
        self.dense_connections = [[] if dst is None else to_list(dst) for dst in to_list(dense_connections, num_layers)]
        self.pad_types = to_list(pad_type, num_layers)
        self.dilations = to_list(dilation, num_layers)
        self.strides = to_list(stride, num_layers)
        self.pool_types = to_list(pool_type, num_layers)
        self.pool_sizes = to_list(pool_size, num_layers)
        self.pool_strides = self.pool_sizes if pool_stride is None else to_list(pool_stride, num_layers)
        self.return_pool_indices = return_pool_indices
        self.return_state = return_state
        self.activation_fn = list(to_list(activation_fn, num_layers + 1))
        self.norm = list(to_list(norm, num_layers + 1))
        self.gated = to_list(gated, num_layers)
        self.pre_activation = pre_activation
        if input_layer:
            assert not isinstance(activation_fn, (list, tuple)) or activation_fn[0] == 'identity'
            assert not isinstance(norm, (list, tuple)) or norm[0] is None
            self.activation_fn[0], self.norm[0] = 'identity', None
        if output_layer:
            assert not isinstance(gated, (list, tuple)) or not gated[-1]
            assert not isinstance(activation_fn, (list, tuple)) or activation_fn[-1] == 'identity'
            assert not isinstance(norm, (list, tuple)) or norm[-1] is None
            self.gated[-1], self.activation_fn[-1], self.norm[-1] = False, 'identity', None

        layer_in_channels = [in_channels] + copy(out_channels)
        shift = int(not pre_activation)
        convs = []
        for i in range(num_layers):
            for dst_idx in self.dense_connections[i]:
                assert dst_idx > i, (i, dst_idx)
                layer_in_channels[dst_idx] += layer_in_channels[i]
            layer_norm = self.norm[i + shift]
            convs.append(self.conv_cls(
                in_channels=layer_in_channels[i], out_channels=self.out_channels[i], kernel_size=self.kernel_sizes[i], dropout=dropout,
                dilation=self.dilations[i], stride=self.strides[i], pad_type=self.pad_types[i], norm=layer_norm,
                norm_kwargs=None if layer_norm is None else norm_kwargs, activation_fn=self.activation_fn[i + shift],
                pre_activation=pre_activation, gated=self.gated[i], return_state=return_state))
        self.convs = nn.ModuleList(convs)

        skips = {}
        for src_idx, destinations in enumerate(self.residual_connections):
            assert len(set(destinations)) == len(destinations), destinations
            for dst_idx in destinations:
                assert dst_idx > src_idx, (src_idx, dst_idx)
                if layer_in_channels[dst_idx] != layer_in_channels[src_idx]:
                    skip_norm = self.norm[src_idx if pre_activation else dst_idx] if normalize_skip_convs else None
                    skips[f'{src_idx}->{dst_idx}'] = self.conv_cls(
                        in_channels=layer_in_channels[src_idx], out_channels=layer_in_channels[dst_idx], kernel_size=1, dropout=dropout,
                        dilation=1, stride=1, pad_type=None, norm=skip_norm, norm_kwargs=None if skip_norm is None else norm_kwargs,
                        activation_fn='identity', pre_activation=pre_activation, gated=False)
        self.residual_skip_convs = nn.ModuleDict(skips)
        self.layer_in_channels = layer_in_channels

        self.input_norm = self.input_activation_fn = self.output_norm = self.output_activation_fn = None
        if self.norm[0] is not None and not pre_activation:
            kwargs = _finalize_norm_kwargs({} if norm_kwargs is None else norm_kwargs, self.norm[0], self.in_channels, False)
            self.input_norm = Normalization(**kwargs)
            self.input_activation_fn = map_activation_fn(self.activation_fn[0])
        if self.norm[-1] is not None and pre_activation:
            kwargs = _finalize_norm_kwargs({} if norm_kwargs is None else norm_kwargs, self.norm[-1], layer_in_channels[-1], False)
            self.output_norm = Normalization(**kwargs)
            self.output_activation_fn = map_activation_fn(self.activation_fn[-1])
        self.reset_parameters()

    @classmethod
    def is_transpose(cls):
        return False

    @classmethod
    def is_2d(cls):
        return False

    def reset_parameters(self):
        for fn in (self.input_activation_fn, self.output_activation_fn):
            if isinstance(fn, nn.PReLU):
                with torch.no_grad():
                    fn.weight.fill_(0.25)
        for i in range(self.num_layers):
            if i == self.num_layers - 1 and self.pre_activation:
                output_activation_fn = self.output_activation_fn
            else:
                output_activation_fn = self.convs[i + self.pre_activation].activation_fn
            self.convs[i].reset_parameters(output_activation_fn)
        for conv in self.residual_skip_convs.values():
            conv.reset_parameters('linear')

    def freeze(self, num_layers=None, freeze_norm_stats=True):
        num_layers = len(self.convs) if num_layers is None else min(num_layers, len(self.convs))
        if num_layers == 0:
            return
        assert num_layers > 0, num_layers
        if self.input_norm is not None:
            self.input_norm.freeze(freeze_stats=freeze_norm_stats)
        if isinstance(self.input_activation_fn, nn.PReLU):
            self.input_activation_fn.weight.requires_grad = False
        for i in range(num_layers):
            self.convs[i].freeze(freeze_norm_stats=freeze_norm_stats)
        for key, conv in self.residual_skip_convs.items():
            if int(key.split('->')[1]) <= num_layers:
                conv.freeze(freeze_norm_stats=freeze_norm_stats)
        if num_layers >= len(self.convs):
            if self.output_norm is not None:
                self.output_norm.freeze(freeze_stats=freeze_norm_stats)
            if isinstance(self.output_activation_fn, nn.PReLU):
                self.output_activation_fn.weight.requires_grad = False

    def _all_lengths(self, lengths):
        """Every length vector the call will meet: the input's and, per layer, behind the convolution and behind the pool."""
        out = [lengths]
        for i, conv in enumerate(self.convs):
            lengths = conv.get_output_sequence_lengths(lengths)
            out.append(lengths)
            if self.pool_sizes[i] > 1:
                lengths = compute_conv_output_sequence_lengths(lengths, self.pool_sizes[i], 1, self.pad_types[i], self.pool_strides[i])
                out.append(lengths)
        return out

    def forward(self, x, sequence_lengths=None, target_shape=None, target_sequence_lengths=None, pool_indices=None, state=None):
        assert x.dim() == 3, x.shape
        if state is not None:
            raise NotImplementedError('CNN1d: state (the streaming mode) is not built')
        assert target_shape is None, target_shape
        assert target_sequence_lengths is None, target_sequence_lengths
        assert pool_indices is None, pool_indices
        sequence_lengths = host_lengths(sequence_lengths)
        table = LengthTable(x.device, [] if sequence_lengths is None else self._all_lengths(sequence_lengths))
        pool_indices = [None] * self.num_layers
        skip_signals = []
        for i, conv in enumerate(self.convs):
            if i == 0 and self.input_norm is not None:
                x = _norm_act(self.input_norm, self.input_activation_fn, x, sequence_lengths, table)
            skip_signals.append(x if self.residual_connections[i] + self.dense_connections[i] else None)
            # the skip signals follow this layer's stride; none of that depends on the layer's output, so it comes first and the first
            # residual connection that ends here is the convolution's own residual operand
            if self.strides[i] > 1:
                for src_idx, x_ in enumerate(skip_signals):
                    if x_ is not None:
                        skip_signals[src_idx] = Pool1d('avg', self.strides[i], pad_type=self.pad_types[i])(x_)[0]
            has_dense = any(x_ is not None and i + 1 in self.dense_connections[src] for src, x_ in enumerate(skip_signals))
            residuals = []
            for src_idx, x_ in enumerate(skip_signals):
                if x_ is not None and i + 1 in self.residual_connections[src_idx]:
                    if f'{src_idx}->{i + 1}' in self.residual_skip_convs:
                        x_, _ = self.residual_skip_convs[f'{src_idx}->{i + 1}'](x_, _table=table)
                    residuals.append(x_)
            fused = residuals.pop(0) if residuals and not has_dense else None
            x, sequence_lengths = conv(x, sequence_lengths=sequence_lengths, _table=table, _residual=fused)
            for src_idx, x_ in enumerate(skip_signals):
                if x_ is not None and i + 1 in self.dense_connections[src_idx]:
                    size = x_.shape[2] - x.shape[2]
                    assert size >= 0, size
                    x = torch.cat((x, x_[..., :x.shape[2]]), dim=1)
            for x_ in residuals:
                assert x_.shape == x.shape, (x_.shape, x.shape)
                a, B, T = _ops.rows(x)
                x = _ops.unrows(_ops.add(a, _ops.rows(x_)[0], B, T), B, T)
            for src_idx in range(len(skip_signals)):
                destinations = self.dense_connections[src_idx] + self.residual_connections[src_idx]
                if destinations and max(destinations) <= i + 1:
                    skip_signals[src_idx] = None
            if i == self.num_layers - 1 and self.output_norm is not None:
                x = _norm_act(self.output_norm, self.output_activation_fn, x, sequence_lengths, table)
            if self.pool_sizes[i] > 1:
                assert self.pool_types[i] is not None
                x, sequence_lengths, pool_indices[i] = Pool1d(self.pool_types[i], self.pool_sizes[i], self.pool_strides[i],
                                                              self.pad_types[i])(x, sequence_lengths)
                for src_idx, x_ in enumerate(skip_signals):
                    if x_ is not None:
                        skip_signals[src_idx] = Pool1d('avg', self.pool_strides[i], pad_type=self.pad_types[i])(x_)[0]
        outputs = [x, sequence_lengths]
        if self.return_pool_indices:
            outputs.append(pool_indices)
        return tuple(outputs)

    @classmethod
    def get_transpose_config(cls, config, transpose_config=None):
        raise NotImplementedError('CNN1d.get_transpose_config: the transposed stack (CNNTranspose1d) is not built')

    def get_shapes(self, input_shape=None, target_shape=None):
        assert (input_shape is None) ^ (target_shape is None), (input_shape, target_shape)
        forward = input_shape is not None
        cur = input_shape if forward else target_shape
        shapes = [cur]
        layers = list(enumerate(self.convs))
        for i, conv in layers if forward else reversed(layers):
            if forward:
                cur = conv.get_output_shape(cur)
                cur[1] = self.layer_in_channels[i + 1]          # with dense connections a layer's channels exceed its convolution's
            else:
                cur = np.copy(cur)
                cur[1] = conv.out_channels
                cur = conv.get_input_shape(cur)
            if self.pool_types[i] is not None:
                cur = compute_conv_output_shape(cur, out_channels=cur[1], kernel_size=self.pool_sizes[i], dilation=1,
                                                stride=self.pool_strides[i], pad_type=self.pad_types[i], transpose=not forward)
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
                                                           pad_type=self.pad_types[i], transpose=not forward)
            seq_lens.append(cur)
        return seq_lens if forward else seq_lens[::-1]

    def get_receptive_field(self):
        receptive_field = np.ones(1).astype(int)
        for i in reversed(range(self.num_layers)):
            receptive_field *= np.array(self.pool_strides[i])
            receptive_field += np.array(self.pool_sizes[i]) - np.array(self.pool_strides[i])
            receptive_field *= np.array(self.strides[i])
            receptive_field += 1 + (np.array(self.kernel_sizes[i]) - 1) * self.dilations[i] - np.array(self.strides[i])
        return receptive_field
