"""The transformer encoder of ``padertorch/contrib/mk/modules/transformer.py`` on the MI355X: the reference's class names, constructor
signatures, parameter and buffer names (a reference ``state_dict`` loads with ``strict=True``) and ``finalize_dogmatic_config``.

What runs where:

    Linear                   ``ops.linear`` (split-fp16 GEMM)
    RoPE, q / k RMS norm,    ``ops.mk_attention.qk_prepare``: one launch for queries and keys between the projections and the scores
      l2_normalization
    the attention            ``ops.mk_attention.bias_attention``: a float ``key_padding_mask`` and ``linear_attention_bias`` are added to the
                             scores inside the kernel; the ``[B, H, Tq, Tk]`` bias is never written
    LayerNorm, RMSNorm,      ``ops.mk_attention.row_norm``; inside ``TransformerEncoderLayer`` the residual add in front of a norm is
      DynamicTanh            part of the norm's launch
    PositionalEncoding       one add of the ``pe`` buffer; dropout: ``nn.Dropout``; the activation: torch's

Two behaviours of the reference are KEPT: with ``is_causal=True`` the attention drops the padding mask AND the linear bias (:291-292,
:960), and ``MultiheadAttention.reset_parameters`` zeroes every 1-D parameter, the RMS weights included (:642-645).

``TransformerEncoder`` hands the layers the sequence lengths as a device vector instead of the reference's dense log-mask, so padded
key tiles are skipped; ``MultiheadAttention`` still takes a float ``key_padding_mask [B, S]`` (it becomes the kernel's ``key_bias``).
Not ported (``NotImplementedError`` naming the option): ``magnitude_preserving``, ``add_bias_kv``, ``flash_attention=True``,
``cond_dim`` / conditioning, ``normalize_skip_connections``, odd head sizes and head sizes above ``ops.attention.MAX_HEAD``, and
``pre_norm=False`` / ``norm=None`` / ``norm='rms'`` in ``TransformerEncoderLayer`` (the reference itself fails there) and
``is_causal=True`` with ``Tq != Tk`` (the reference's causal mask is aligned top-left, the kernels' bottom-right); the decoder classes and ``PositionalConvEmbedding`` are not here, ``NORM_MAP`` has no ``batch1d``.
"""
import copy
import functools
import math
from collections import namedtuple

import torch
import torch.nn.functional as F
from torch import nn
from torch.utils.checkpoint import checkpoint as activation_checkpoint

from .... import _lib
from ....base import Module
from ....ops import attention as _attn
from ....ops import gemm as _gemm
from ....ops import mk_attention as _mk
from ....ops.linear import linear as _linear
from ....ops.mappings import ACTIVATION_FN_MAP, _CallableDispatcher

__all__ = ['Linear', 'PositionalEncoding', 'RoPE', 'DynamicTanh', 'LayerNorm', 'RMSNorm', 'NORM_MAP', 'ScaledDotProductAttention',
           'ATTENTION_FN_MAP', 'MultiheadAttention', 'TransformerNormBlock', 'EncoderLayer', 'TransformerEncoderLayer',
           'TransformerEncoder', 'NormOutputs', 'GELU', 'positional_embedding']

NormOutputs = namedtuple('NORM_OUTPUTS', ['x', 'layer_scale'], defaults=[1])


def _unsupported(**options):
    for name, value in options.items():
        if value:
            raise NotImplementedError(f'{name}={value!r} is not ported to the HIP path')


def positional_embedding(d_model, max_len=5000):
    """The reference's table (:47-56): ``sin`` on the even, ``cos`` on the odd columns, frequencies ``max_len^(-i / half)``."""
    position = torch.arange(max_len).unsqueeze(1)
    half = d_model // 2
    div_term = torch.exp(torch.arange(0, half) * (-math.log(float(max_len)) / half))
    pe = torch.zeros(max_len, 1, d_model)
    pe[:, 0, 0::2] = torch.sin(position * div_term)
    pe[:, 0, 1::2] = torch.cos(position * div_term)
    return pe


class GELU(nn.GELU):
    """``contrib/mk/modules/activations.py``'s GELU: what ``finalize_dogmatic_config`` names as the activation."""

    def __init__(self, approximate='none', magnitude_preserving=False):
        _unsupported(magnitude_preserving=magnitude_preserving)
        super().__init__(approximate=approximate)
        self.magnitude_preserving = magnitude_preserving


class Linear(Module):
    """``x W^T + b`` over the last axis through ``ops.linear`` (:59-110)."""

    def __init__(self, in_features, out_features, bias=True, magnitude_preserving=False, chunks=None, generator=None):
        super().__init__()
        _unsupported(magnitude_preserving=magnitude_preserving)
        self.in_features, self.out_features = in_features, out_features
        self.magnitude_preserving = magnitude_preserving
        self.chunks = chunks
        self.weight = nn.Parameter(nn.init.xavier_uniform_(torch.empty(out_features, in_features), generator=generator))
        if bias:
            self.bias = nn.Parameter(torch.zeros(out_features))
        else:
            self.register_parameter('bias', None)

    def forward(self, x):
        _lib.require_gpu(x)
        if not _gemm.usable(x, self.weight):                # the library-GEMM A/B mode, other dtypes: said, never silent
            _lib.leaving_native_path(f'a contrib.mk Linear({self.in_features}, {self.out_features}) layer',
                                     'ops.gemm.ENABLED = False or an input that is not fp32')
            return F.linear(x, self.weight, self.bias)
        return _linear(self, x.reshape(-1, x.shape[-1])).view(*x.shape[:-1], self.out_features)


class PositionalEncoding(Module):
    """``x + pe[:T]`` and dropout (:113-148)."""

    def __init__(self, d_model, dropout=0., max_len=5000, batch_first=True):
        super().__init__()
        self.dropout = nn.Dropout(p=dropout)
        self.batch_first = batch_first
        pe = positional_embedding(d_model, max_len)
        self.register_buffer('pe', pe.transpose(0, 1) if batch_first else pe)

    def reset_parameters(self):
        return self

    def forward(self, x):
        x = x + (self.pe[:, :x.size(1)] if self.batch_first else self.pe[:x.size(0)])
        return self.dropout(x)


class RoPE(Module):
    """Rotary positional embedding (:231-270) for ``x [B, (H,) T, d]``: positions start at 1, ``theta = max_len^(-2i/d)`` repeated in
    pairs (the ``theta`` buffer, read by the kernel), pairs ``(2i, 2i+1)`` rotated.  Alone it is one ``qk_prepare`` launch; inside
    ``MultiheadAttention`` it is a stage of the launch that prepares q and k."""

    def __init__(self, d_model, max_len=10_000, batch_first=True):
        super().__init__()
        if d_model % 2:
            raise NotImplementedError(f'RoPE: odd d_model={d_model} has no rotary pairs')
        self.batch_first = batch_first
        theta = max_len ** (-2 * torch.arange(d_model // 2) / d_model)
        self.register_buffer('theta', torch.repeat_interleave(theta, 2)[None, None])

    def forward(self, x):
        if x.dim() not in (3, 4):
            raise ValueError(f'RoPE: x [B, (H,) T, d], got {tuple(x.shape)}')
        T, d = x.shape[-2:]
        out, _ = _mk.qk_prepare(x.reshape(-1, T, 1, d), theta=self.theta)
        return out.view(x.shape)


class LayerNorm(nn.LayerNorm):
    """``nn.LayerNorm`` returning ``NormOutputs(x, None)`` (:363-456), unconditioned."""

    def __init__(self, normalized_shape, eps=1e-5, elementwise_affine=True, bias=True, device=None, dtype=None, cond_dim=None,
                 activation_fn=None, layer_scale=False, zero_init=False, magnitude_preserving=False):
        _unsupported(cond_dim=cond_dim, magnitude_preserving=magnitude_preserving)
        super().__init__(normalized_shape=normalized_shape, eps=eps, elementwise_affine=elementwise_affine, bias=bias, device=device,
                         dtype=dtype)
        if len(self.normalized_shape) != 1:
            raise NotImplementedError(f'LayerNorm: normalized_shape={normalized_shape!r}: the last axis only')
        self.magnitude_preserving = magnitude_preserving
        self.shift = bias
        self.layer_scale = layer_scale
        self.cond_layer = None

    def add_norm(self, x, res=None):
        return _mk.row_norm('layer', x, res, self.weight, self.bias, eps=self.eps)

    def forward(self, x, cond=None):
        _unsupported(cond_dim=cond is not None)
        return NormOutputs(self.add_norm(x), None)


class RMSNorm(nn.RMSNorm):
    """``nn.RMSNorm`` over the last axis (the reference's ``NORM_MAP['rms']``) on ``row_norm``; returns the tensor, as ``nn.RMSNorm`` does."""

    def add_norm(self, x, res=None):
        if len(self.normalized_shape) != 1:
            raise NotImplementedError(f'RMSNorm: normalized_shape={self.normalized_shape!r}: the last axis only')
        return _mk.row_norm('rms', x, res, self.weight, eps=self.eps)

    def forward(self, x):
        return self.add_norm(x)


class DynamicTanh(Module):
    """Dynamic tanh ``tanh(alpha x) weight + bias`` (:459-537), unconditioned; returns ``NormOutputs(x, None)``."""

    def __init__(self, num_features, alpha_init_value=0.5, elementwise_affine=True, bias=True, cond_dim=None, activation_fn=None,
                 layer_scale=False, zero_init=False):
        super().__init__()
        _unsupported(cond_dim=cond_dim)
        self.num_features = num_features
        self.alpha = nn.Parameter(torch.ones(1) * alpha_init_value)
        self.elementwise_affine = elementwise_affine
        if elementwise_affine:
            self.weight = nn.Parameter(torch.ones(num_features))
            self.bias = nn.Parameter(torch.zeros(num_features))
        self.shift = bias
        self.layer_scale = layer_scale
        self.cond_layer = None

    def add_norm(self, x, res=None):
        affine = self.elementwise_affine
        return _mk.row_norm('dyt', x, res, self.weight if affine else None, self.bias if affine else None, self.alpha)

    def forward(self, x, cond=None):
        _unsupported(cond_dim=cond is not None)
        return NormOutputs(self.add_norm(x), None)


NORM_MAP = _CallableDispatcher(
    layer=LayerNorm,
    adaln=functools.partial(LayerNorm, elementwise_affine=False),
    rms=RMSNorm,
    dyt=DynamicTanh,
)


class ScaledDotProductAttention(Module):
    """``softmax(q k^T / sqrt(d) + attn_mask) v`` for ``q, k, v [B, H, T, d]`` (:273-355); returns ``(out, None)``.  ``attn_mask`` is the
    float key mask ``[B, S]`` or ``[B, 1, 1, S]``; ``lengths`` (device int vector) and ``slopes [H]`` are the kernel's forms of the
    padding mask and the linear bias.  As in the reference, ``is_causal=True`` applies the causal mask ALONE; it needs ``Tq == Tk``
    (``NotImplementedError`` otherwise: the reference aligns the mask top-left, ``j <= i``, the kernels bottom-right)."""

    def __init__(self, *args, enable_flash=None, enable_mem_efficient=None, magnitude_preserving=False, **kwargs):
        super().__init__()
        _unsupported(magnitude_preserving=magnitude_preserving)
        self.enable_flash = enable_flash
        self.enable_mem_efficient = enable_mem_efficient
        self.magnitude_preserving = magnitude_preserving

    def forward(self, q, k, v, attn_mask=None, is_causal=False, lengths=None, slopes=None):
        if is_causal:
            if q.shape[-2] != k.shape[-2]:
                # F.scaled_dot_product_attention(is_causal=True) (:292) aligns the mask top-left (j <= i); the kernels align it
                # bottom-right (j <= i + Tk - Tq, ops.attention): the same only for Tq == Tk
                raise NotImplementedError(f'is_causal=True with Tq != Tk ({q.shape[-2]}, {k.shape[-2]}) is not ported: the kernels\' causal '
                                          f'mask ends on the last key, the reference\'s starts on the first')
            return _mk.bias_attention(q, k, v, causal=True), None
        if attn_mask is not None:
            if attn_mask.dim() == 4 and attn_mask.shape[1:3] == (1, 1):
                attn_mask = attn_mask[:, 0, 0]
            if attn_mask.dim() != 2 or not attn_mask.is_floating_point():
                raise NotImplementedError(f'attn_mask: a float key mask [B, S] or [B, 1, 1, S], got {attn_mask.dtype} {tuple(attn_mask.shape)}')
        # also without a bias: this path's backward forms its row term from the recomputed probabilities (csrc/attention.hip,
        # attn_delta_bias_kernel), which the small query / key gradients behind an RMS norm need
        return _mk.bias_attention(q, k, v, lengths, attn_mask, slopes), None


ATTENTION_FN_MAP = _CallableDispatcher(scaled_dot_product=ScaledDotProductAttention)


class MultiheadAttention(Module):
    """https://arxiv.org/abs/1706.03762 (:549-763), self and cross attention (``kdim``, ``vdim``, ``Tq != Tk``).  ``forward(query, key,
    value, key_padding_mask=None, is_causal=False)`` returns ``(y, None)``.  ``key_padding_mask``: the reference's float log-mask
    ``[B, S]`` (added to the scores inside the kernel; ``-inf`` hides a key) or an int32 / int64 DEVICE vector ``[B]`` of key counts -
    what ``TransformerEncoder`` passes - which lets the kernel skip padded key tiles.

    Kept from the reference: ``is_causal=True`` drops the padding mask AND the linear bias; ``reset_parameters`` zeroes every 1-D
    parameter, the RMS weights of ``q_norm`` / ``k_norm`` included.  ``is_causal=True`` is ported for ``Tq == Tk`` only
    (``NotImplementedError`` under cross attention of unequal lengths, see ``ScaledDotProductAttention``).  An odd head size raises
    only together with ``rope``, ``rms_norm`` or ``l2_normalization`` (the pair-wise kernel); plain attention takes any head size."""

    def __init__(self, embed_dim, num_heads, dropout=0., bias=True, add_bias_kv=False, kdim=None, vdim=None,
                 attention_fn='scaled_dot_product', batch_first=True, magnitude_preserving=False, l2_normalization=False,
                 flash_attention=False, rope=False, rms_norm=False, linear_attention_bias=False, **kwargs):
        super().__init__()
        assert batch_first, "Only batch_first=True is supported"
        _unsupported(magnitude_preserving=magnitude_preserving, add_bias_kv=add_bias_kv, flash_attention=flash_attention)
        assert embed_dim % num_heads == 0, (embed_dim, num_heads)
        dh = embed_dim // num_heads
        if dh % 2 and (rope or rms_norm or l2_normalization):
            raise NotImplementedError(f'embed_dim / num_heads = {dh}: an odd head size is not ported (the rotary pairs)')
        if dh > _attn.MAX_HEAD:
            raise NotImplementedError(f'embed_dim / num_heads = {dh} is beyond the fused attention kernels\' MAX_HEAD = {_attn.MAX_HEAD}')
        self.embed_dim = embed_dim
        self.num_heads = num_heads
        self.attention_fn = ATTENTION_FN_MAP[attention_fn](embed_dim, num_heads, magnitude_preserving=magnitude_preserving, **kwargs)
        self.lin_query = Linear(embed_dim, embed_dim, bias=bias)
        self.lin_key = Linear(kdim or embed_dim, embed_dim, bias=bias)
        self.lin_value = Linear(vdim or embed_dim, embed_dim, bias=bias)
        self.out_proj = Linear(embed_dim, embed_dim, bias=bias)
        self.dropout = nn.Dropout(dropout)
        self.l2_normalization = l2_normalization
        self.flash_attention = flash_attention
        self.add_bias_kv = add_bias_kv
        self.bias_k = self.bias_v = None
        self.rope = RoPE(dh, batch_first=batch_first) if rope else None
        if rms_norm:
            self.q_norm = RMSNorm(dh)
            self.k_norm = RMSNorm(dh)
        else:
            self.q_norm = self.k_norm = None
        self.linear_attention_bias = linear_attention_bias

    def reset_parameters(self, seed=None):
        generator = torch.Generator(device=self.out_proj.weight.device)
        if seed is not None:
            generator.manual_seed(seed)
        for param in self.parameters():
            if param.ndim == 1:
                nn.init.zeros_(param)                       # biases - and the RMS weights, as in the reference
            elif param.ndim == 2:
                nn.init.xavier_uniform_(param, generator=generator)
            else:
                raise ValueError(f"Unexpected parameter shape: {param.shape}")

    def forward(self, query, key, value, key_padding_mask=None, is_causal=False):
        B, Tq, _ = query.shape
        Tk, H, dh = key.shape[1], self.num_heads, self.embed_dim // self.num_heads
        q = self.lin_query(query).view(B, Tq, H, dh)
        k = self.lin_key(key).view(B, Tk, H, dh)
        v = self.lin_value(value).view(B, Tk, H, dh)
        if self.q_norm is not None or self.rope is not None or self.l2_normalization:
            rms = self.q_norm is not None
            q, k = _mk.qk_prepare(q, k, self.q_norm.weight if rms else None, self.k_norm.weight if rms else None,
                                  None if self.rope is None else self.rope.theta, self.l2_normalization,
                                  self.q_norm.eps if rms else None)
        lengths = key_bias = None
        if key_padding_mask is not None:
            if key_padding_mask.is_floating_point():
                key_bias = key_padding_mask
            else:
                lengths = _attn.device_lengths(key_padding_mask, query.device)
        slopes = _mk.linear_slopes(H, query.device) if self.linear_attention_bias else None
        x, weights = self.attention_fn(q.transpose(1, 2), k.transpose(1, 2), v.transpose(1, 2), attn_mask=key_bias, is_causal=is_causal,
                                       lengths=lengths, slopes=slopes)
        x = x.transpose(1, 2).reshape(B, Tq, self.embed_dim)        # a view: the kernel wrote [B, Tq, H, dh]
        return self.dropout(self.out_proj(x)), weights


class TransformerNormBlock(Module):
    """``NORM_MAP[norm](d_model)`` (:766-784).  ``forward`` returns what the norm returns; ``add_norm(x, res)`` returns ``(x + res, norm(x +
    res))`` from one launch."""

    def __init__(self, norm, d_model, cond_dim=None):
        super().__init__()
        _unsupported(cond_dim=cond_dim)
        self.norm = NORM_MAP[norm](d_model)

    def add_norm(self, x, res):
        return self.norm.add_norm(x, res)

    def forward(self, inputs, cond=None):
        _unsupported(cond_dim=cond is not None)
        return self.norm(inputs)


class EncoderLayer(Module):
    """The feed-forward half of a layer and its norms (:787-896)."""

    def __init__(self, d_model, dim_feedforward=2048, dropout=0., activation='relu', norm='layer', output_norm=None,
                 magnitude_preserving=False, bias=True, pre_activation=False, cond_dim=None):
        super().__init__()
        _unsupported(magnitude_preserving=magnitude_preserving, cond_dim=cond_dim)
        self.d_model = d_model
        self.activation = activation
        self.magnitude_presering = magnitude_preserving
        activation_fn = ACTIVATION_FN_MAP[activation]
        try:
            activation_fn = activation_fn()
        except TypeError:
            pass                                            # already instantiated
        self.mlp = self.build_mlp(d_model, dim_feedforward, activation_fn, dropout=dropout, bias=bias, pre_activation=pre_activation)
        if norm is None:
            self.sa_norm = self.mlp_norm = None
        else:
            self.sa_norm = TransformerNormBlock(norm, d_model, cond_dim)
            self.mlp_norm = TransformerNormBlock(norm, d_model, cond_dim)
        self.output_norm = None if output_norm is None else TransformerNormBlock(output_norm, d_model)

    def build_mlp(self, d_model, dim_feedforward, activation_fn, dropout=0., bias=True, magnitude_preserving=False, pre_activation=False):
        layers = [Linear(d_model, dim_feedforward, bias=bias), activation_fn, Linear(dim_feedforward, d_model, bias=bias),
                  nn.Dropout(dropout)]
        return nn.Sequential(*([activation_fn] if pre_activation else []), *layers)

    def reset_parameters(self, seed=None):
        generator = torch.Generator(device=self.mlp[-2].weight.device)
        if seed is not None:
            generator.manual_seed(seed)
        gain = torch.nn.init.calculate_gain(self.activation) if isinstance(self.activation, str) else 1.0
        for param in self.mlp.parameters():
            if param.ndim > 1:
                nn.init.xavier_uniform_(param, gain=gain, generator=generator)
            else:
                nn.init.zeros_(param)

    def forward(self, x):
        raise NotImplementedError('EncoderLayer is the base of TransformerEncoderLayer')


class TransformerEncoderLayer(EncoderLayer):
    """Self-attention and feed-forward blocks, pre-norm (:899-1024).  ``forward(x, padding_mask=None)``: ``padding_mask`` is what
    ``MultiheadAttention`` takes as ``key_padding_mask``.  Every ``x + sublayer(x)`` that a norm follows is one launch with it.
    ``pre_norm=False`` and ``norm=None`` raise ``NotImplementedError``: the reference's own forward raises a ``TypeError`` for both
    (``F.softplus`` of the int ``layer_scale = 1``, :970), so there is no behaviour to reproduce.  ``norm='rms'`` raises too: the
    reference unpacks the bare tensor ``nn.RMSNorm`` returns along the batch axis (``output_norm='rms'`` works, there and here)."""

    def __init__(self, d_model, attention_fn, activation, nhead=1, dim_feedforward=2048, dropout=0., norm='layer', output_norm=None,
                 bidirectional=True, magnitude_preserving=False, bias=True, pre_activation=False, cond_dim=None,
                 normalize_skip_connections=False, pre_norm=True):
        _unsupported(normalize_skip_connections=normalize_skip_connections)
        if not pre_norm or norm is None:
            # the reference's forward raises there (:1006-1008, :970: softplus of the int layer_scale = 1), so there is nothing to port
            raise NotImplementedError(f'pre_norm={pre_norm!r}, norm={norm!r}: the reference layer runs pre-norm with a norm only')
        super().__init__(d_model, dim_feedforward, dropout, activation, norm, output_norm=output_norm, bias=bias,
                         magnitude_preserving=magnitude_preserving, pre_activation=pre_activation, cond_dim=cond_dim)
        if not isinstance(self.sa_norm.norm, (LayerNorm, DynamicTanh)):
            # the reference unpacks the norm's NormOutputs (:1003); nn.RMSNorm returns a bare tensor, which that unpacking splits along
            # the batch axis: an error unless B == 2, a wrong result when it is
            raise NotImplementedError(f'norm={norm!r}: a norm that returns NormOutputs (layer, adaln, dyt) only')
        self.nhead = nhead
        self.attention_fn = attention_fn
        self.normalize_skip_connections = normalize_skip_connections
        self.pre_norm = pre_norm
        self.bidirectional = bidirectional

    @classmethod
    def finalize_dogmatic_config(cls, config):
        config["attention_fn"] = {
            'factory': MultiheadAttention,
            'attention_fn': 'scaled_dot_product',
            'embed_dim': config['d_model'],
            'num_heads': config['nhead'],
            'dropout': config['dropout'],
            'magnitude_preserving': config['magnitude_preserving'],
            'bias': config["bias"],
        }
        config['activation'] = {
            'factory': GELU,
            'magnitude_preserving': config['magnitude_preserving'],
        }

    def _call_attention(self, q, padding_mask, *, k=None, v=None, attention_fn=None):
        k = q if k is None else k
        v = k if v is None else v
        attention_fn = self.attention_fn if attention_fn is None else attention_fn
        h, _ = attention_fn(q, k, v, key_padding_mask=padding_mask if self.bidirectional else None, is_causal=not self.bidirectional)
        return h

    def reset_parameters(self, seed=None):
        try:
            self.attention_fn.reset_parameters(seed=seed)
        except AttributeError:
            pass
        super().reset_parameters(seed=seed)

    def forward(self, x, padding_mask=None, latent_cond=None):
        _unsupported(cond_dim=latent_cond is not None)
        h = self._call_attention(self.sa_norm(x).x, padding_mask)
        h, o = self.mlp_norm.add_norm(h, x)                 # h = x + attention, o = mlp_norm(h): one launch
        o = self.mlp(o)
        if self.output_norm is not None:                    # (the reference returns what the norm returns here, :1022-1023)
            y = self.output_norm.add_norm(o, h)[1]
            return y if isinstance(self.output_norm.norm, RMSNorm) else NormOutputs(y, None)
        return h + o


class TransformerEncoder(Module):
    """Feature projection, positional encoding, ``num_layers`` copies of ``encoder_layer`` and the input / output norms (:1127-1250).
    ``forward(x, sequence_lengths=None)`` returns ``(y, sequence_lengths)``.  The lengths go to the layers as ONE device vector
    (``ops.attention.device_lengths``) instead of the reference's ``[B, T]`` log-mask."""

    def __init__(self, input_size, encoder_layer, feature_extractor=None, num_layers=6, input_norm=None, output_norm=None,
                 positional_encoding=None, dropout=0., mlp_head=None, use_activation_checkpointing=True, zero_init=False):
        super().__init__()
        self.input_size = input_size
        self.mlp_head = mlp_head
        if feature_extractor is None and input_size != encoder_layer.d_model:
            self.feature_extractor = Linear(input_size, encoder_layer.d_model)
        else:
            self.feature_extractor = feature_extractor
        self.positional_encoding = nn.Identity() if positional_encoding is None else positional_encoding
        self.input_norm = NormOutputs if input_norm is None else NORM_MAP[input_norm](encoder_layer.d_model)
        self.output_norm = NormOutputs if output_norm is None else NORM_MAP[output_norm](encoder_layer.d_model)
        self.dropout = nn.Dropout(dropout)
        self.use_activation_checkpointing = use_activation_checkpointing
        self.layers = nn.ModuleList([])
        for _ in range(num_layers):
            layer = copy.deepcopy(encoder_layer)
            layer.reset_parameters()
            self.layers.append(layer)
        if zero_init:
            self.zero_init_()

    @classmethod
    def finalize_dogmatic_config(cls, config):
        config['encoder_layer'] = {'factory': TransformerEncoderLayer}
        config['positional_encoding'] = {'d_model': config['encoder_layer']['d_model']}

    def __getitem__(self, item):
        return self.layers[item]

    def zero_init_(self):
        if self.mlp_head is not None:
            for param in self.mlp_head.parameters():
                param.detach().zero_()
            return True
        return False

    def reset_parameters(self, seed=None):
        try:
            self.positional_encoding.reset_parameters(seed=seed)
        except (AttributeError, TypeError):
            pass
        for layer in self.layers:
            layer.reset_parameters(seed=seed)

    def _forward(self, x, sequence_lengths=None, *, latent_cond=None):
        _unsupported(cond_dim=latent_cond is not None)
        if self.feature_extractor is not None:
            x = self.feature_extractor(x)
        h = self.positional_encoding(x)
        h = self.dropout(self.input_norm(h).x)
        lengths = _attn.device_lengths(sequence_lengths, h.device)
        for layer in self.layers:
            h = layer(h, padding_mask=lengths)
            if isinstance(h, NormOutputs):
                h = h.x
        o = self.output_norm(h).x
        return (o if self.mlp_head is None else self.mlp_head(o)), sequence_lengths

    def forward(self, x, sequence_lengths=None, *, cond=None):
        if self.use_activation_checkpointing:
            return activation_checkpoint(self._forward, x, sequence_lengths, latent_cond=cond, use_reentrant=False)
        return self._forward(x, sequence_lengths, latent_cond=cond)
