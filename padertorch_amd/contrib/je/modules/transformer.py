"""The transformer encoder stack of ``padertorch/contrib/je/modules/transformer.py`` on the MI355X: ``MultiHeadAttention``,
``TransformerLayer``, ``TransformerLayerStack`` and ``get_causal_mask`` with the reference's constructor arguments (the ``queue_size``
spelling included), ``forward`` signatures, return values and parameter names, so a reference ``state_dict`` loads with ``strict=True``.

What runs where:

    the dense layers        ``torch.nn.Linear`` modules called through ``ops.linear`` (split-fp16 GEMM); the projections of one input
                            share one measurement of its range; a ReLU ``activation_ff`` runs in the hidden GEMM's epilogue
    the attention           ``ops.attention.attention`` (``csrc/attention.hip``): the projections' ``[B, T, H, dh]`` output is read in place,
                            the ``[B, H, Tq, Tk]`` scores are never written; ``TransformerLayer`` does not ask for the weights
    norm='layer'            ``ops.attention.norm_residual``: masked LayerNorm + residual in one launch, either ``norm_first`` order
    norm='batch' / None     the ``Normalization`` module (``csrc/norm.hip``) and a plain add
    positional encoding     ``ops.attention.positional_encoding_`` in place on the input projection
    dropout > 0 (training)  ``F.dropout`` where the reference calls it - a library kernel, the one exception

Departures from the reference: the attention weights ``MultiHeadAttention`` returns carry no gradient, and ``d_model / num_heads <= 128``.
"""
import torch
import torch.nn.functional as F

from ....base import Module
from ....modules.normalization import Normalization
from ....ops import attention as _attn
from ....ops import gemm as _gemm
from ....ops.linear import linear as _linear, release_input as _release_input, share_input as _share_input
from ....ops.mappings import ACTIVATION_FN_MAP

__all__ = ['scaled_dot_product_attention', 'MultiHeadAttention', 'TransformerLayer', 'TransformerLayerStack', 'get_causal_mask']

scaled_dot_product_attention = _attn.scaled_dot_product_attention


def get_causal_mask(x):
    """``tril`` of ones like ``x [..., Tq, Tk]`` with the diagonal ``Tk - Tq``: query ``i`` sees keys ``j <= i + Tk - Tq`` (:259-260)."""
    return torch.tril(torch.ones_like(x), diagonal=(x.shape[-1] - x.shape[-2]))


def _project(module, x, x_range=None, activation=None):
    """``module(x)`` for ``x [B, T, C]`` through ``ops.linear``; ``x_range``: the device word with ``max |x|`` when the caller has it."""
    B, T, C = x.shape
    return _linear(module, x.reshape(B * T, C), x_range=x_range, activation=activation).view(B, T, module.out_features)


def _range_of(x, module):
    """``max |x|`` as the device word the GEMM's operand packing takes, measured ONCE for all the projections of ``x`` (None where
    ``ops.linear`` measures nothing: CPU tensors, the library-GEMM mode)."""
    return _gemm.absmax(x) if _gemm.usable(x, module.weight) else None


class MultiHeadAttention(Module):
    """https://arxiv.org/abs/1706.03762 (transformer.py:41-88).  ``forward(q, k, v, seq_len=None, mask=None)`` returns ``(y, weights)``;
    with ``need_weights=False`` the second value is ``None`` and the weights kernel is not launched.  Mask precedence as in
    ``ops.attention.scaled_dot_product_attention``: a causal layer (``bidirectional=False``) ignores ``seq_len``."""

    def __init__(self, queue_size, key_size, value_size, d_model, output_size, num_heads=8, bidirectional=False):
        super().__init__()
        assert d_model % num_heads == 0, (d_model, num_heads)
        self.queue_size = queue_size
        self.d_model = d_model
        self.output_size = output_size
        self.num_heads = num_heads
        self.bidirectional = bidirectional
        self.lin_queue = torch.nn.Linear(queue_size, self.d_model)
        self.lin_key = torch.nn.Linear(key_size, self.d_model)
        self.lin_value = torch.nn.Linear(value_size, self.d_model)
        self.out = torch.nn.Linear(self.d_model, self.output_size)

    def forward(self, q, k, v, seq_len=None, mask=None, need_weights=True):
        B, Tq, _ = q.shape
        Tk = k.shape[1]
        H, dh = self.num_heads, self.d_model // self.num_heads
        if dh > _attn.MAX_HEAD:
            raise NotImplementedError(f'MultiHeadAttention: d_model / num_heads = {dh} is beyond the fused attention kernels\' limit of '
                                      f'{_attn.MAX_HEAD}')
        # one range measurement and ONE operand packing per distinct input: self-attention projects one tensor three times, attention
        # over a state or a memory one tensor twice
        q2 = q.reshape(B * Tq, -1)
        k2 = q2 if k is q else k.reshape(B * Tk, -1)
        v2 = k2 if v is k else v.reshape(B * Tk, -1)
        r_q = _range_of(q2, self.lin_queue)
        r_k = r_q if k2 is q2 else _range_of(k2, self.lin_key)
        r_v = r_k if v2 is k2 else _range_of(v2, self.lin_value)
        if v2 is k2:
            _share_input(k2)
        try:
            qh = _linear(self.lin_queue, q2, x_range=r_q).view(B, Tq, H, dh).transpose(1, 2)
            kh = _linear(self.lin_key, k2, x_range=r_k).view(B, Tk, H, dh).transpose(1, 2)
            vh = _linear(self.lin_value, v2, x_range=r_v).view(B, Tk, H, dh).transpose(1, 2)
        finally:
            _release_input(k2)
        lengths = _attn.device_lengths(seq_len, q.device) if self.bidirectional else None
        x, weights = _attn.attention(qh, kh, vh, lengths, not self.bidirectional, mask, need_weights)
        x = x.transpose(1, 2).reshape(B, Tq, self.d_model)          # a view: the kernel wrote [B, Tq, H, dh]
        return _project(self.out, x), weights


def _fusable(norm):
    """The layer norm ``ops.attention.norm_residual`` restates: over the channels of ``btc``, shift and scale, ``gamma`` and ``beta``."""
    return (norm is not None and norm.statistics_axis == (2,) and norm.shift and norm.scale and norm.gamma is not None
            and norm.beta is not None and norm.batch_axis == 0 and norm.sequence_axis == 1)


class TransformerLayer(Module):
    """https://arxiv.org/abs/1706.03762 (transformer.py:91-175).  ``forward(x, seq_len, m=None, seq_len_m=None, state=None)`` returns
    ``(y, s)`` with ``s = cat(state, x)`` the keys and values of the self-attention (``state`` needs a causal layer)."""

    def __init__(self, d_model=512, d_ff=2048, num_heads=8, bidirectional=True, cross_attention=False, norm='layer', norm_kwargs={},
                 norm_first=True, activation_ff='relu', dropout=.0):
        super().__init__()
        self.multi_head_self_attention = MultiHeadAttention(d_model, d_model, d_model, d_model, d_model, num_heads=num_heads,
                                                            bidirectional=bidirectional)
        self.cross_attention = cross_attention
        self.hidden = torch.nn.Linear(d_model, d_ff)
        self.out = torch.nn.Linear(d_ff, d_model)
        if norm is None:
            self.self_attention_norm = None
            self.output_norm = None
        else:
            norm_kwargs = {"data_format": 'btc', "shape": (None, None, d_model), 'eps': 1e-2, **norm_kwargs}
            if norm == 'batch':
                norm_kwargs['statistics_axis'] = 'bt'
            elif norm == 'layer':
                norm_kwargs['statistics_axis'] = 'c'
            else:
                raise ValueError(f'{norm} normalization not known.')
            self.self_attention_norm = Normalization(**norm_kwargs)
            self.output_norm = Normalization(**norm_kwargs)
        if cross_attention:
            self.multi_head_cross_attention = MultiHeadAttention(d_model, d_model, d_model, d_model, d_model, num_heads=num_heads,
                                                                 bidirectional=True)
            self.cross_attention_norm = None if norm is None else Normalization(**norm_kwargs)
        self.norm_first = norm_first
        self.relu_ff = activation_ff == 'relu'
        self.activation_ff = ACTIVATION_FN_MAP[activation_ff]()
        self.dropout = dropout

    def _dropout(self, h):
        return F.dropout(h, self.dropout) if self.training and self.dropout > 0. else h

    def _norm_residual(self, norm, h, x, seq_len):
        """``norm(h) + x`` (``norm_first``) or ``norm(h + x)``; plain ``h + x`` without a norm (:151-155)."""
        if norm is None:
            return h + x
        if _fusable(norm) and h.is_cuda and h.dtype == torch.float32:
            return _attn.norm_residual(h, x, norm.gamma, norm.beta, _attn.device_lengths(seq_len, h.device), norm.eps, self.norm_first)
        if self.norm_first:
            return norm(h, sequence_lengths=seq_len) + x
        return norm(h + x, sequence_lengths=seq_len)

    def forward(self, x, seq_len, m=None, seq_len_m=None, state=None):
        if state is not None:
            assert self.multi_head_self_attention.bidirectional is False
        s = x if state is None else torch.cat((state, x), 1)
        h, _ = self.multi_head_self_attention(x, s, s, seq_len=seq_len, need_weights=False)
        h = self._norm_residual(self.self_attention_norm, self._dropout(h), x, seq_len)
        if self.cross_attention:
            assert m is not None
            q = h
            h, _ = self.multi_head_cross_attention(q, m, m, seq_len=seq_len_m, need_weights=False)
            h = self._norm_residual(self.cross_attention_norm, self._dropout(h), q, seq_len)        # seq_len, not seq_len_m (:163)
        if self.relu_ff:
            y = _project(self.hidden, h, activation='relu')
        else:
            y = self.activation_ff(_project(self.hidden, h))
        y = _project(self.out, y)
        y = self._norm_residual(self.output_norm, self._dropout(y), h, seq_len)
        return y, s


class TransformerLayerStack(Module):
    """The input projection, the positional encoding and ``num_layers`` layers (transformer.py:178-256).  ``forward(x, seq_len, m=None,
    seq_len_m=None, state=None)`` returns ``(y, states)``; ``seq_len`` may be a host list or an int32 / int64 device vector (device data:
    nothing is read back, so a forward + backward can be captured in a graph and replayed with other lengths)."""

    def __init__(self, input_size, hidden_size=512, d_ff=2048, num_heads=8, num_layers=6, bidirectional=False, cross_attention=False,
                 norm='layer', norm_kwargs={}, norm_first=True, activation_ff='relu', dropout=0., positional_encoding=True):
        super().__init__()
        self.positional_encoding = positional_encoding
        self.dropout = dropout
        self.num_layers = num_layers
        self.lin = torch.nn.Linear(input_size, hidden_size)
        self.transformer_layers = torch.nn.ModuleList([
            TransformerLayer(hidden_size, d_ff, num_heads, bidirectional=bidirectional, cross_attention=cross_attention, norm=norm,
                             norm_kwargs=norm_kwargs, norm_first=norm_first, activation_ff=activation_ff, dropout=dropout)
            for _ in range(num_layers)])

    def add_positional_encoding(self, x):
        b, t, d = x.shape
        assert d % 2 == 0, x.shape
        return _attn.positional_encoding_(x if x.is_contiguous() else x.contiguous())

    def forward(self, x, seq_len, m=None, seq_len_m=None, state=None):
        h = _project(self.lin, x)
        if self.positional_encoding:
            h = self.add_positional_encoding(h)
        if state is None:
            state = len(self.transformer_layers) * [None]
        if x.is_cuda:                                       # once for all layers
            seq_len, seq_len_m = _attn.device_lengths(seq_len, x.device), _attn.device_lengths(seq_len_m, x.device)
        for i, layer in enumerate(self.transformer_layers):
            h, state[i] = layer(h, seq_len=seq_len, m=m, seq_len_m=seq_len_m, state=state[i])
        return h, state
