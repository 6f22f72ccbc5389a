"""``CNN`` and ``CRNN`` of ``padertorch/contrib/je/modules/hybrid.py``: a ``CNN2d`` front end, a ``CNN1d`` behind it and, in ``CRNN``, a GRU and
a dense stack, with the reference's constructors, attributes and submodule names (``cnn_2d`` / ``cnn_1d``; ``_cnn_2d``, ``_cnn_1d``,
``_rnn``, ``_fcn``), so a reference ``state_dict`` loads with ``strict=True``.

    CNN.forward(x [B, C, F, T], sequence_lengths=None, condition=None) -> (y [B, C', T'], sequence_lengths[, pool indices])
    CRNN.forward(x [B, C, F, T], seq_len=None) -> (y [B, T', K], seq_len)

Between the stacks ``b c f t -> b (c f) t`` is ONE gather launch from the 2-D stack's rows ``[B F T, C]`` into the rows ``[B T, C F]``
that ``CNN1d`` reads in place.  The positional encoding and the ``condition`` are input preparation, built with torch indexing and
``cat`` as in the reference.  ``CRNN`` runs its ``torch.nn.GRU`` through the GRU kernel as ``rnn.py``'s wrapper does (lengths in any
order, zeros behind them, which is what ``pad_packed_sequence`` gives) and its ``fcn`` is this package's ``fully_connected_stack``.

There is no ``Configurable`` system here (``base.py``): ``finalize_dogmatic_config`` fills a plain dict with the reference's defaults
under what the caller set, and ``from_config`` instantiates its ``{'factory': ..., **kwargs}`` nodes.

Not built (``NotImplementedError``): ``state`` / ``return_state``, ``get_transpose_config`` and ``CNNTranspose``, an ``rnn`` that is
neither a ``torch.nn.GRU`` / ``LSTM`` nor ``None``.
"""
import torch
from torch import nn

from ....base import _instantiate
from ....modules.fully_connected import fully_connected_stack
from ....ops import je_conv as _ops
from ....ops import je_conv2d as _ops2
from ....ops import seq_pool as _seq
from .conv import CNN1d
from .conv2d import CNN2d
from .rnn import RNN

__all__ = ['CNN', 'CRNN']


def stack_channels(x):
    """``x [B, C, F, T]`` -> ``[B, C F, T]``: one gather from the rows ``[B F T, C]`` to the rows ``[B T, C F]``, returned as their view."""
    r, B, F_, T = _ops2.planes(x)
    C = r.shape[1]
    if r.stride(0) != C:
        r = _seq.rows_layout(r.unsqueeze(0)).squeeze(0)
    # out[b, t, c, f] = r[b, f, t, c]: the axes (t, c) of the source collapse into one of stride 1
    out = _seq.rows_layout(r.as_strided((B, T * C, F_), (F_ * T * C, 1, T * C)))
    return _ops.unrows(out.view(B * T, C * F_), B, T)


def _fill(config, key, defaults):
    """The reference's ``config[key] = defaults`` of a dogmatic config: defaults UNDER what the caller set; an explicit None stays."""
    if key in config and config[key] is None:
        return
    config[key] = {**defaults, **config.get(key, {})}


def _make(node):
    return None if node is None else _instantiate(node)


class _Configured:
    @classmethod
    def from_config(cls, config):
        """The module of a (partial) config dict: ``finalize_dogmatic_config``, then every ``{'factory': ...}`` node instantiated."""
        config = {k: (dict(v) if isinstance(v, dict) else v) for k, v in config.items() if k != 'factory'}
        cls.finalize_dogmatic_config(config)
        return cls(**{k: _make(v) if isinstance(v, dict) and 'factory' in v else v for k, v in config.items()})


class CNN(_Configured, nn.Module):
    """Combines ``CNN2d`` and ``CNN1d`` sequentially."""
    def __init__(self, cnn_2d: CNN2d, cnn_1d: CNN1d, *, input_height=None, positional_encoding=False, conditional_dims=0,
                 return_pool_indices=False, return_state=False):
        super().__init__()
        if return_state:
            raise NotImplementedError('CNN: return_state (the streaming mode) is not built')
        assert cnn_2d.return_pool_indices == cnn_1d.return_pool_indices == return_pool_indices, (
            cnn_2d.return_pool_indices, cnn_1d.return_pool_indices, return_pool_indices)
        self.cnn_2d = cnn_2d
        self.cnn_1d = cnn_1d
        self.input_height = input_height
        self.positional_encoding = positional_encoding
        self.conditional_dims = conditional_dims
        self.return_pool_indices = return_pool_indices
        self.return_state = return_state

    def add_positional_encoding(self, x):
        b, c, f, t = x.shape
        encoding = torch.broadcast_to(torch.linspace(0, 1, f, device=x.device)[:, None], (b, 1, f, t))
        return torch.cat([x, encoding], dim=1)

    def add_condition(self, x, condition):
        if condition.dim() == 2:
            condition = condition.unsqueeze(-1)
        if x.dim() == 3:
            assert condition.dim() == 3, condition.shape
            return torch.cat([x, torch.broadcast_to(condition, (x.shape[0], condition.shape[1], x.shape[2]))], dim=1)
        if x.dim() == 4:
            b, _, f, t = x.shape
            if condition.dim() == 3:
                condition = condition.unsqueeze(2)
            assert condition.dim() == 4, condition.shape
            return torch.cat([x, torch.broadcast_to(condition, (b, condition.shape[1], f, t))], dim=1)
        raise ValueError('x must be 3- or 4- dimensional')

    def forward(self, x, sequence_lengths=None, condition=None, state=None):
        assert x.dim() == 4, x.shape
        if state is not None:
            raise NotImplementedError('CNN: state (the streaming mode) is not built')
        if self.positional_encoding:
            x = self.add_positional_encoding(x)
        if condition is not None:
            x = self.add_condition(x, condition)
        x, sequence_lengths, *more = self.cnn_2d(x, sequence_lengths)
        pool_indices_2d = more[0] if self.cnn_2d.return_pool_indices else None
        x = stack_channels(x)
        if condition is not None:
            x = self.add_condition(x, condition)
        x, sequence_lengths, *more = self.cnn_1d(x, sequence_lengths)
        pool_indices_1d = more[0] if self.cnn_1d.return_pool_indices else None
        outputs = [x, sequence_lengths]
        if self.return_pool_indices:
            outputs.append((pool_indices_2d, pool_indices_1d))
        return tuple(outputs)

    @classmethod
    def finalize_dogmatic_config(cls, config):
        for key, value in (('input_height', None), ('positional_encoding', False), ('conditional_dims', 0), ('return_pool_indices', False),
                           ('return_state', False)):
            config.setdefault(key, value)
        shared = {'return_pool_indices': config['return_pool_indices'], 'return_state': config['return_state']}
        _fill(config, 'cnn_2d', {'factory': CNN2d, **shared})
        _fill(config, 'cnn_1d', {'factory': CNN1d, **shared})
        if config['input_height'] is not None:
            cnn_2d = _make(config['cnn_2d'])
            _, out_channels, output_size, _ = cnn_2d.get_shapes((1, config['cnn_2d']['in_channels'], config['input_height'], 1000))[-1]
            config['cnn_1d']['in_channels'] = int(out_channels * output_size + config['conditional_dims'])

    @classmethod
    def get_transpose_config(cls, config, transpose_config=None):
        raise NotImplementedError('CNN.get_transpose_config: a transposed hybrid (CNNTranspose) is not built; conv_transpose.get_transpose_config '
                                  'mirrors a CNN1d / CNN2d')

    def get_shapes(self, in_shape):
        cnn_2d_shapes = self.cnn_2d.get_shapes(in_shape)
        out_shape = cnn_2d_shapes[-1]
        return cnn_2d_shapes, self.cnn_1d.get_shapes((out_shape[0], out_shape[1] * out_shape[2], out_shape[3]))

    def get_seq_lens(self, in_lengths):
        cnn_2d_lengths = self.cnn_2d.get_sequence_lengths(in_lengths)
        return cnn_2d_lengths, self.cnn_1d.get_sequence_lengths(cnn_2d_lengths[-1])


class CRNN(_Configured, nn.Module):
    """``CNN2d -> CNN1d -> GRU -> fcn`` (each may be ``None``)."""
    input_size_key = 'input_size'

    def __init__(self, cnn_2d: CNN2d, cnn_1d: CNN1d, rnn, fcn, *, post_rnn_pooling=None, input_size=None):
        super().__init__()
        RNN(rnn)                                            # (refuses what the recurrence kernels do not cover, here and not in the first call)
        self.input_size = input_size
        self._cnn_2d = cnn_2d
        self._cnn_1d = cnn_1d
        self._rnn = rnn
        self._fcn = fcn
        self._post_rnn_pooling = post_rnn_pooling

    def cnn_2d(self, x, seq_len=None):
        if self._cnn_2d is not None:
            x, seq_len = self._cnn_2d(x, seq_len)
        if x.dim() != 3:
            assert x.dim() == 4
            x = stack_channels(x)
        return x, seq_len

    def cnn_1d(self, x, seq_len=None):
        if self._cnn_1d is not None:
            x, seq_len = self._cnn_1d(x, seq_len)
        return x, seq_len

    def rnn(self, x, seq_len=None):
        if self._rnn is not None:
            x, _ = RNN(self._rnn).train(self.training)(x, seq_len)         # a wrapper around the very module: the GRU kernel with lengths
        return x.transpose(1, 2)

    def post_rnn_pooling(self, x, seq_len):
        if self._post_rnn_pooling is not None:
            x, seq_len = self._post_rnn_pooling(x, seq_len)
        return x, seq_len

    def fcn(self, x):
        return x if self._fcn is None else self._fcn(x)

    def forward(self, x, seq_len=None):
        x, seq_len = self.cnn_2d(x, seq_len)
        x, seq_len = self.cnn_1d(x, seq_len)
        x = self.rnn(x, seq_len=seq_len)
        x, seq_len = self.post_rnn_pooling(x, seq_len)
        return self.fcn(x), seq_len

    @classmethod
    def finalize_dogmatic_config(cls, config):
        config.setdefault('post_rnn_pooling', None)
        config.setdefault(cls.input_size_key, None)
        _fill(config, 'cnn_2d', {'factory': CNN2d})
        _fill(config, 'cnn_1d', {'factory': CNN1d})
        _fill(config, 'rnn', {'factory': nn.GRU})
        _fill(config, 'fcn', {'factory': fully_connected_stack})
        input_size = config[cls.input_size_key]
        if config['cnn_2d'] is not None and input_size is not None:
            cnn_2d = _make(config['cnn_2d'])
            output_size = cnn_2d.get_shapes((1, config['cnn_2d']['in_channels'], input_size, 1000))[-1][2]
            input_size = int(cnn_2d.out_channels[-1] * output_size)
        if config['cnn_1d'] is not None:
            if input_size is not None:
                config['cnn_1d']['in_channels'] = input_size
            input_size = config['cnn_1d']['out_channels'][-1]
        if config['rnn'] is not None:
            if config['rnn']['factory'] == nn.GRU:
                config['rnn'].update({'num_layers': 1, 'bias': True, 'batch_first': True, 'dropout': 0., 'bidirectional': False})
            if input_size is not None:
                config['rnn']['input_size'] = input_size
            input_size = config['rnn']['hidden_size']
        if config['fcn'] is not None:
            config['fcn']['input_size'] = input_size
