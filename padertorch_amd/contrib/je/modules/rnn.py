"""The sequence wrappers of ``padertorch/contrib/je/modules/rnn.py`` on the MI355X: ``RNN``, ``GRU``, ``LSTM``, ``TransformerEncoder`` and
``reverse_sequence`` with the reference's constructor, call, ``freeze`` and ``finalize_dogmatic_config`` defaults.  ``rnn`` is a
``torch.nn.GRU``, a ``torch.nn.LSTM``, this package's ``TransformerLayerStack`` or ``None``: the parameters are the torch module's own,
so a reference ``state_dict`` loads with ``strict=True``; only the arithmetic moves.

    forward(x [B, F, T], seq_len) -> (y [B, D H, T], seq_len)

What runs where:

    b f t -> b t f          ONE copy, by the gather kernel of ``ops.seq_pool`` (``rows_layout``; with ``reverse=True`` for the LSTM and the
                            transformer the same launch is the ``reverse_sequence``).  A ``[B, F, T]`` tensor has no 2-D view with
                            rows ``(b, t)``, so the first projection GEMM cannot read it in place.
    b t f -> b f t          no copy: ``y`` is the transposed VIEW of the last layer's ``[B T, D H]`` output, as the reference's
                            ``rearrange`` returns it
    torch.nn.GRU            ``ops.gru.chunk_gru`` layer by layer over the table ``(b T, 1, len_b)`` built on the device; ``reverse=True``
                            is the kernels' ``flip``: no reversal of the activation at all
    torch.nn.LSTM           ``ops.dprnn.chunk_lstm_params`` layer by layer over the same table; ``reverse=True``: ``reverse_sequence``
                            before and after
    TransformerLayerStack   called as it is; ``reverse=True`` as for the LSTM
    dropout > 0 (training)  ``F.dropout`` between the layers, where ``torch.nn.GRU`` places it - a library kernel, the one exception

Lengths may come in any order (the reference's ``pack_padded_sequence`` insists on descending ones), as a list, numpy array, CPU tensor
or CUDA int32 / int64 tensor; CUDA lengths are read by the kernels only, so forward + backward capture in a graph that serves other
lengths.  The output of the recurrent layers is zero behind each length, which is what ``pad_packed_sequence`` gives.

Not built (``NotImplementedError``, no library fallback): ``output_net`` from a config (the reference's ``CNN1d`` / ``CNNTranspose1d`` of
``contrib/je/modules/conv.py`` do not exist here; a module passed to the constructor is called as ``output_net(x, seq_len)``), initial and
final states (the reference's wrapper passes none and discards them), ``proj_size != 0``, other ``torch.nn.RNNBase`` subclasses, an LSTM
without biases, and hidden sizes beyond the kernels' bounds (GRU 1792, LSTM 1536).
"""
import torch
import torch.nn.functional as F
from torch import nn

from ....ops import dprnn as _dprnn
from ....ops import gru as _gru
from ....ops import seq_pool as _pool
from .transformer import TransformerLayerStack

__all__ = ['RNN', 'GRU', 'LSTM', 'TransformerEncoder', 'reverse_sequence']

reverse_sequence = _pool.reverse_sequence


def _layer_params(rnn, layer):
    """``(w_ih, w_hh, b_ih, b_hh)`` of the forward and, if any, the reverse direction of one layer; absent tensors are None."""
    out = []
    for suffix in ('', '_reverse') if rnn.bidirectional else ('',):
        for name in ('weight_ih', 'weight_hh', 'bias_ih', 'bias_hh'):
            out.append(getattr(rnn, f'{name}_l{layer}{suffix}') if rnn.bias or name.startswith('weight') else None)
    return out + [None] * (8 - len(out))


def _supported(rnn):
    if rnn is None or isinstance(rnn, TransformerLayerStack):
        return
    if not isinstance(rnn, (nn.GRU, nn.LSTM)):
        raise NotImplementedError(f'RNN: rnn is a torch.nn.GRU, a torch.nn.LSTM, a TransformerLayerStack or None; {type(rnn).__name__} has '
                                  f'no HIP kernel here and there is no library fallback')
    if getattr(rnn, 'proj_size', 0) != 0:
        raise NotImplementedError(f'RNN: proj_size = {rnn.proj_size} is not built (the recurrence kernels have no projection)')
    if isinstance(rnn, nn.LSTM) and not rnn.bias:
        raise NotImplementedError('RNN: a torch.nn.LSTM without biases is not built (ops.dprnn\'s recurrence kernel adds b_hh)')
    bound = _gru.MAX_HIDDEN if isinstance(rnn, nn.GRU) else _dprnn.MAX_HIDDEN
    if rnn.hidden_size > bound:
        raise NotImplementedError(f'RNN: hidden_size {rnn.hidden_size} is beyond the {type(rnn).__name__} recurrence kernels\' bound of '
                                  f'{bound} (the LDS of a compute unit)')


class RNN(nn.Module):
    def __init__(self, rnn, output_net=None, reverse=False):
        super().__init__()
        _supported(rnn)
        self.rnn = rnn
        self.output_net = output_net
        self.reverse = reverse

    def _recurrent(self, rows, table, B, T):
        """The layers of ``self.rnn`` over ``rows [B, T, N]`` (contiguous) -> ``[B, T, D H]``."""
        rnn = self.rnn
        h = rows.view(B * T, rows.shape[2])
        for layer in range(rnn.num_layers):
            params = _layer_params(rnn, layer)
            if isinstance(rnn, nn.GRU):
                h = _gru.chunk_gru(h, table, T, *params, flip=self.reverse)
            else:
                h = _dprnn.chunk_lstm_params(h, table, T, *params)
            if self.training and rnn.dropout > 0. and layer < rnn.num_layers - 1:
                h = F.dropout(h, rnn.dropout)
        return h.view(B, T, h.shape[1])

    def forward(self, x, seq_len):
        if self.rnn is not None:
            if x.dim() != 3:
                raise ValueError(f'RNN: x [B, F, T], got {tuple(x.shape)}')
            B, _, T = x.shape
            lengths = _gru.device_lengths(seq_len, B, x.device)
            x = x.transpose(1, 2)                                       # b t f, a view
            if isinstance(self.rnn, nn.GRU):
                assert self.rnn.batch_first is True, self.rnn.batch_first
                x = self._recurrent(_pool.rows_layout(x), _gru.sequence_table(x, lengths, B, T), B, T)
            else:
                x = reverse_sequence(x, lengths) if self.reverse else _pool.rows_layout(x)
                if isinstance(self.rnn, TransformerLayerStack):
                    x, _ = self.rnn(x, lengths)
                else:
                    assert self.rnn.batch_first is True, self.rnn.batch_first
                    x = self._recurrent(x, _gru.sequence_table(x, lengths, B, T), B, T)
                if self.reverse:
                    x = reverse_sequence(x, lengths)
            x = x.transpose(1, 2)                                       # b f t, a view
        if self.output_net is not None:
            x, seq_len = self.output_net(x, seq_len)
        return x, seq_len

    def freeze(self, num_layers=None):
        if num_layers == 0:
            return
        num_rnn_layers = self.rnn.num_layers if num_layers is None else min(num_layers, self.rnn.num_layers)
        for name, param in self.rnn.named_parameters():
            name_split = name.split('.')
            if name.endswith(f'_l{num_rnn_layers}') or ((len(name_split) > 1) and (name_split[1] == str(num_rnn_layers))):
                break
            param.requires_grad = False
        num_out_layers = None if num_layers is None else max(num_layers - self.rnn.num_layers, 0)
        if self.output_net is not None:
            self.output_net.freeze(num_out_layers)

    @classmethod
    def finalize_dogmatic_config(cls, config):
        if config['output_net'] is not None:
            raise NotImplementedError('RNN: output_net is the reference\'s padertorch.contrib.je.modules.conv.CNN1d, which is not built '
                                      'here; construct the RNN with output_net=None or pass a module of your own to the constructor')


class GRU(RNN):
    @classmethod
    def finalize_dogmatic_config(cls, config):
        config['rnn'] = {
            'factory': nn.GRU,
            'num_layers': 1,
            'bias': True,
            'dropout': 0.,
            'bidirectional': False,
            'batch_first': True,
        }
        assert config['rnn'] is None or config['rnn']['factory'] == nn.GRU, config['rnn']
        super().finalize_dogmatic_config(config)


class LSTM(RNN):
    @classmethod
    def finalize_dogmatic_config(cls, config):
        config['rnn'] = {
            'factory': nn.LSTM,
            'num_layers': 1,
            'bias': True,
            'dropout': 0.,
            'bidirectional': False,
            'batch_first': True,
        }
        assert config['rnn'] is None or config['rnn']['factory'] == nn.LSTM, config['rnn']
        super().finalize_dogmatic_config(config)


class TransformerEncoder(RNN):
    @classmethod
    def finalize_dogmatic_config(cls, config):
        config['rnn'] = {
            'factory': TransformerLayerStack,
            'num_layers': 6,
            'hidden_size': 512,
            'num_heads': 8,
            'd_ff': 2048,
            'bidirectional': False,
            'cross_attention': False,
            'activation_ff': 'relu',
            'dropout': 0.,
            'positional_encoding': True,
        }
        assert config['rnn'] is None or config['rnn']['factory'] == TransformerLayerStack, config['rnn']
        assert config['rnn']['cross_attention'] is False, config['rnn']['cross_attention']
        super().finalize_dogmatic_config(config)
