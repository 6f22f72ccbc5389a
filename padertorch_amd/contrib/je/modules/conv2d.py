"""``Conv2d``, ``CNN2d`` and ``Pool2d`` of ``padertorch/contrib/je/modules/conv.py`` / ``conv_utils.py`` on the MI355X: the 2-D members of
the families in ``conv.py`` (``_Conv``, ``_CNN``), with the reference's constructor arguments, attributes, submodule and parameter names
(``conv`` / ``gate_conv`` are ``torch.nn.Conv2d``, the norms this package's ``Normalization`` with ``data_format='bcft'``), so a reference
``state_dict`` loads with ``strict=True``.  The arithmetic is ``ops.je_conv2d`` (``csrc/je_conv2d.hip``): a direct
convolution on the matrix instructions, no padded copy, no transposing copy between the layers of a ``CNN2d``.

    Conv2d.forward(x [B, C, F, T], sequence_lengths=None) -> (y, sequence_lengths)
    CNN2d.forward(x, sequence_lengths=None) -> (y, sequence_lengths[, pool_indices])
    Pool2d.forward(x, sequence_lengths=None) -> (y, sequence_lengths, pool_indices)

``kernel_size``, ``stride``, ``dilation`` and ``pad_type`` are scalars or pairs ``(f, t)``.  Sequence lengths refer to the ``t`` axis only;
``norm='batch'`` has one group over ``b, f, t``, ``'sequence'`` one per ``(b, f)`` (the reference's ``statistics_axis`` ``'btf'`` / ``'t'``).
What ``conv.py`` lists as not built is not built here either.
"""
import numpy as np
import torch.nn.functional as F
from torch import nn

from ....ops import je_conv2d as _ops2
from .conv import _CNN, _Conv, _norm_operands, _track
from .conv_utils import (LengthTable, _compute_conv_out_size, activation_code, compute_pad_size, host_lengths, to_pair)

__all__ = ['Conv2d', 'CNN2d', 'Pool2d']


class Pool2d(nn.Module):
    """``nn.MaxPool2d`` / ``nn.AvgPool2d`` behind the reference's padding, on ``x [B, C, F, T]``:
    ``forward(x, sequence_lengths=None) -> (y, sequence_lengths, pool_indices)``.  As in the reference the pad sizes are those of a pool
    whose stride is its size (``compute_pad_size(k, 1, k, pad_type)``), whatever ``stride`` says; lengths refer to the ``t`` axis."""
    def __init__(self, pool_type, pool_size, stride=None, pad_type=None):
        super().__init__()
        self.pool_type = pool_type
        self.pool_size = to_pair(pool_size)
        self.stride = self.pool_size if stride is None else to_pair(stride)
        self.pad_type = to_pair(pad_type)

    def geometry(self, plane):
        """``(front pair, output plane)`` for an input plane ``(F, T)``."""
        front, out = [], []
        for n, k, s, p in zip(plane, self.pool_size, self.stride, self.pad_type):
            f, e = compute_pad_size(k, 1, k, p)
            padded = n + f + e
            if padded < k:
                raise ValueError(f'Pool2d: {n} positions (padded: {padded}) are fewer than the pool size {k}')
            front.append(f)
            out.append((padded - k) // s + 1)
        return front, out

    def output_lengths(self, sequence_lengths):
        """The ``t`` lengths behind the pool, as the reference counts them (with the pool's own stride, unlike its pad sizes)."""
        out = _compute_conv_out_size(host_lengths(sequence_lengths), self.pool_size[-1], 1, self.stride[-1], self.pad_type[-1])
        assert all(out > 0), out
        return out

    def forward(self, x, sequence_lengths=None):
        if all(np.array(self.pool_size) < 2):
            return x, sequence_lengths, None
        assert self.pool_type is not None, 'pool_size > 1 not allowed when pool_type is None'
        if self.pool_type not in ('max', 'avg'):
            raise ValueError(f'{self.pool_type} pooling unknown.')
        r, B, F_in, T_in = _ops2.planes(x)
        front, (F_out, T_out) = self.geometry((F_in, T_in))
        y, index = _ops2.pool2d(r, B, (F_in, T_in), (F_out, T_out), self.pool_size, self.stride, front, self.pool_type == 'max')
        if sequence_lengths is not None:
            sequence_lengths = self.output_lengths(sequence_lengths)
        return (_ops2.unplanes(y, B, F_out, T_out), sequence_lengths,
                None if index is None else _ops2.unplanes(index, B, F_out, T_out))


def _repeat(lengths, F_):
    """Every example's length once per frequency row: the ``B F`` "examples" of ``T`` rows the statistics kernels see."""
    return None if lengths is None else np.repeat(lengths, F_)


def _norm_act2d(norm, activation_fn, x, lengths, table):
    """``activation_fn(norm(x))`` on ``x [B, C, F, T]`` (``input_norm`` / ``output_norm``)."""
    from ....ops import je_conv as _ops
    r, B, F_, T = _ops2.planes(x)
    code, p, slope = activation_code(activation_fn)
    kind, fixed = _norm_operands(norm)
    out, stats = _ops.norm_act(r, B * F_, T, kind, norm.eps, code, p, norm.gamma, norm.beta, slope, fixed, table.get(_repeat(lengths, F_)))
    _track(norm, stats)
    return _ops2.unplanes(out, B, F_, T)


class Conv2d(_Conv):
    torch_cls = nn.Conv2d

    def forward(self, x, sequence_lengths=None, state=None, *, _table=None, _residual=None):
        if state is not None:
            raise NotImplementedError('Conv2d: state (the streaming mode) is not built')
        if self.training and self.dropout > 0.:
            x = F.dropout(x, self.dropout)
        r, B, F_in, T_in = _ops2.planes(x)
        lengths = host_lengths(sequence_lengths)
        out_lengths = None if lengths is None else self.get_output_sequence_lengths(lengths)
        F_out, T_out = (int(n) for n in self.get_output_shape((B, self.in_channels, F_in, T_in))[2:])
        norm_lengths = _repeat(lengths, F_in) if self.pre_activation else _repeat(out_lengths, F_out)
        table = LengthTable(x.device, [norm_lengths]) if _table is None else _table
        front = [compute_pad_size(k, d, s, p)[0] for k, d, s, p in zip(self.kernel_size, self.dilation, self.stride, self.pad_type)]
        code, p, slope = activation_code(self.activation_fn)
        kind, fixed = (None, None) if self.norm is None else _norm_operands(self.norm)
        cfg = _ops2.BlockConfig2d(B, F_in, T_in, F_out, T_out, tuple(self.kernel_size), tuple(self.stride), tuple(self.dilation),
                                  tuple(front), kind, 0. if self.norm is None else self.norm.eps, code, p, bool(self.pre_activation))
        res = None
        if _residual is not None:
            res, *plane = _ops2.planes(_residual)
            assert (*plane, res.shape[1]) == (B, F_out, T_out, self.out_channels), (_residual.shape, B, F_out, T_out)
        y, stats = _ops2.conv_block2d(
            r, cfg, self.conv.weight, self.conv.bias, self.gate_conv.weight if self.gated else None,
            self.gate_conv.bias if self.gated else None, None if self.norm is None else self.norm.gamma,
            None if self.norm is None else self.norm.beta, slope, fixed, table.get(norm_lengths) if self.norm is not None else None, res)
        if self.norm is not None:
            _track(self.norm, stats)
        return _ops2.unplanes(y, B, F_out, T_out), out_lengths


class CNN2d(_CNN):
    conv_cls = Conv2d
    pool_cls = Pool2d
    _norm_act = staticmethod(_norm_act2d)

    @staticmethod
    def _add(x, x_):
        from ....ops import je_conv as _ops
        a, B, F_, T = _ops2.planes(x)
        return _ops2.unplanes(_ops.add(a, _ops2.planes(x_)[0], B * F_, T), B, F_, T)

    def _all_lengths(self, lengths, shape):
        """Every repeated length vector the call will meet: the ``t`` lengths once per frequency row at the input, behind every
        convolution and behind every pool (one upload for all of them)."""
        F_ = int(shape[2])
        out = [_repeat(lengths, F_)]
        for i, conv in enumerate(self.convs):
            lengths = conv.get_output_sequence_lengths(lengths)
            F_ = int(_compute_conv_out_size(F_, conv.kernel_size[0], conv.dilation[0], conv.stride[0], conv.pad_type[0]))
            out.append(_repeat(lengths, F_))
            size, stride, pad = to_pair(self.pool_sizes[i]), to_pair(self.pool_strides[i]), to_pair(self.pad_types[i])
            if any(np.array(size) > 1):
                lengths = _compute_conv_out_size(lengths, size[1], 1, stride[1], pad[1])
                F_ = (F_ + sum(compute_pad_size(size[0], 1, size[0], pad[0])) - size[0]) // stride[0] + 1
                out.append(_repeat(lengths, F_))
        return out
