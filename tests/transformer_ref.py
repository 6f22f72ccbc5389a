"""An fp64 restatement of the transformer encoder stack in plain torch (CPU), written from the formulas of
``padertorch/contrib/je/modules/transformer.py``: what the GPU tests compare against at shapes the fixture
tests/golden/g24_transformer.npz does not hold.  tests/test_transformer_host.py pins it to the fixture (1e-12 of max|want|).

    scaled_dot_product_attention(q, k, v, seq_len, bidirectional, mask)   scores, the three masks in the reference's precedence, softmax
    MultiHeadAttention, TransformerLayer, TransformerLayerStack          the classes, parameter names as in the reference
    masked_norm(x, gamma, beta, axes, seq_len, eps)                       Normalization's training-mode forward
    positional_encoding(t, d)                                             [t, d], interleaved cos / sin
    variant_stack(config), run_variant(g, name)                           a fixture variant's stack / its fp64 run on the fixture's inputs

One thing is NOT "the formula": the reference builds the positional encoding from ``torch.arange`` (int64) and a python float, so its
angles ``t / 10000^(2i/d)`` and their cos / sin are float32 tensors even in an fp64 run.  The restatement (and the kernel) take the angle
the same way; the fixture could not be met to 1e-12 otherwise.
"""
import json
import math
from pathlib import Path

import numpy as np
import torch

VALUE, GRAD = 1e-5, 2e-4
GOLDEN = Path(__file__).resolve().parent / 'golden' / 'g24_transformer.npz'


_GOLDEN = None


def golden():
    """The index file and every ``g24_transformer_<variant>.npz`` behind it as ONE dict, loaded once (the arrays are never written)."""
    global _GOLDEN
    if _GOLDEN is None:
        g = dict(np.load(GOLDEN, allow_pickle=False))
        g['variants'] = json.loads(str(g['variants']))
        for name in g['variants']:
            g.update(np.load(GOLDEN.with_name(f'g24_transformer_{name}.npz'), allow_pickle=False))
        _GOLDEN = g
    return _GOLDEN


def rel_dev(got, want):
    got = torch.as_tensor(got).detach().cpu().double()
    want = torch.as_tensor(want).detach().cpu().double()
    assert got.shape == want.shape, (got.shape, want.shape)
    nan = torch.isnan(want)
    assert torch.equal(torch.isnan(got), nan), 'NaN positions differ'
    if nan.all():
        return 0.
    return float((got - want)[~nan].abs().max() / want[~nan].abs().max().clamp(min=1e-300))


def length_mask(x, seq_len, batch_axis=0, sequence_axis=1):
    if seq_len is None:
        return torch.ones_like(x)
    lengths = torch.as_tensor(seq_len).long()
    sb, st = [1] * x.dim(), [1] * x.dim()
    sb[batch_axis % x.dim()] = -1
    st[sequence_axis % x.dim()] = -1
    return (torch.arange(x.shape[sequence_axis]).reshape(st) < lengths.reshape(sb)).to(x.dtype).expand(x.shape)


def get_causal_mask(x):
    tq, tk = x.shape[-2:]
    i = torch.arange(tq)[:, None]
    j = torch.arange(tk)[None, :]
    return (j <= i + tk - tq).to(x.dtype).expand(x.shape)


def log_mask(mask):
    return torch.where(mask > 0, torch.zeros((), dtype=torch.float64), torch.full((), -math.inf, dtype=torch.float64))


def scaled_dot_product_attention(q, k, v, seq_len=None, bidirectional=False, mask=None):
    y = q @ k.transpose(-2, -1) / math.sqrt(k.shape[-1])
    if mask is not None:
        y = y + log_mask(mask.expand(y.shape))
    if not bidirectional:
        y = y + log_mask(get_causal_mask(y))
    elif seq_len is not None:
        y = y + log_mask(length_mask(y, seq_len, 0, -1))
    y = torch.softmax(y, dim=-1)
    return y @ v, y


def masked_norm(x, gamma, beta, axes, seq_len, eps):
    mask = length_mask(x, seq_len, 0, 1)
    n = mask.sum(axes, keepdim=True).clamp(min=1)
    xm = x * mask
    mean = xm.sum(axes, keepdim=True) / n
    var = ((xm ** 2).sum(axes, keepdim=True) / n - mean ** 2).clamp(min=0.)
    return ((xm - mean) / torch.sqrt(var + eps) * gamma + beta) * mask


def positional_encoding(t, d):
    positions = torch.arange(t)[:, None]
    dimensions = torch.arange(d // 2)
    angle = positions / (10000 ** (2 * dimensions / d))             # float32, as in the reference
    return torch.stack((torch.cos(angle), torch.sin(angle)), dim=-1).reshape(t, d)


class Norm(torch.nn.Module):
    """``Normalization(data_format='btc', shape=(None, None, d), statistics_axis=..., eps=1e-2)`` in training mode."""

    def __init__(self, d, kind, eps=1e-2):
        super().__init__()
        self.axes = (2,) if kind == 'layer' else (0, 1)
        self.eps = eps
        self.gamma = torch.nn.Parameter(torch.ones(1, 1, d))
        self.beta = torch.nn.Parameter(torch.zeros(1, 1, d))
        if kind == 'batch':
            self.register_buffer('num_tracked_values', torch.zeros(1, 1, d))
            self.register_buffer('running_mean', torch.zeros(1, 1, d))
            self.register_buffer('running_power', torch.ones(1, 1, d))

    def forward(self, x, seq_len):
        return masked_norm(x, self.gamma, self.beta, self.axes, seq_len, self.eps)


class MultiHeadAttention(torch.nn.Module):
    def __init__(self, queue_size, key_size, value_size, d_model, output_size, num_heads=8, bidirectional=False):
        super().__init__()
        self.d_model, self.num_heads, self.bidirectional = d_model, num_heads, bidirectional
        self.lin_queue = torch.nn.Linear(queue_size, d_model)
        self.lin_key = torch.nn.Linear(key_size, d_model)
        self.lin_value = torch.nn.Linear(value_size, d_model)
        self.out = torch.nn.Linear(d_model, output_size)

    def forward(self, q, k, v, seq_len=None, mask=None):
        B, Tq, Tk, H = q.shape[0], q.shape[1], k.shape[1], self.num_heads

        def heads(x, T):
            return x.view(B, T, H, self.d_model // H).transpose(1, 2)
        x, w = scaled_dot_product_attention(heads(self.lin_queue(q), Tq), heads(self.lin_key(k), Tk), heads(self.lin_value(v), Tk),
                                            seq_len=seq_len, bidirectional=self.bidirectional, mask=mask)
        return self.out(x.transpose(1, 2).reshape(B, Tq, self.d_model)), w


ACTIVATIONS = dict(relu=torch.relu, tanh=torch.tanh, sigmoid=torch.sigmoid, elu=torch.nn.functional.elu, identity=lambda x: x)


class TransformerLayer(torch.nn.Module):
    def __init__(self, d_model=512, d_ff=2048, num_heads=8, bidirectional=True, cross_attention=False, norm='layer', norm_first=True,
                 activation_ff='relu'):
        super().__init__()
        if norm not in (None, 'layer', 'batch'):
            raise ValueError(f'{norm} normalization not known.')
        self.multi_head_self_attention = MultiHeadAttention(d_model, d_model, d_model, d_model, d_model, num_heads, bidirectional)
        self.cross_attention = cross_attention
        self.hidden = torch.nn.Linear(d_model, d_ff)
        self.out = torch.nn.Linear(d_ff, d_model)
        self.self_attention_norm = None if norm is None else Norm(d_model, norm)
        self.output_norm = None if norm is None else Norm(d_model, norm)
        if cross_attention:
            self.multi_head_cross_attention = MultiHeadAttention(d_model, d_model, d_model, d_model, d_model, num_heads, True)
            self.cross_attention_norm = None if norm is None else Norm(d_model, norm)
        self.norm_first = norm_first
        self.activation_ff = activation_ff

    def _join(self, norm, h, x, seq_len):
        if norm is None:
            return h + x
        return norm(h, seq_len) + x if self.norm_first else norm(h + x, seq_len)

    def forward(self, x, seq_len, m=None, seq_len_m=None, state=None):
        if state is not None:
            assert self.multi_head_self_attention.bidirectional is False
        s = x if state is None else torch.cat((state, x), 1)
        h, _ = self.multi_head_self_attention(x, s, s, seq_len=seq_len)
        h = self._join(self.self_attention_norm, h, x, seq_len)
        if self.cross_attention:
            q = h
            h, _ = self.multi_head_cross_attention(q, m, m, seq_len=seq_len_m)
            h = self._join(self.cross_attention_norm, h, q, seq_len)
        y = self.out(ACTIVATIONS[self.activation_ff](self.hidden(h)))
        return self._join(self.output_norm, y, h, seq_len), s


class TransformerLayerStack(torch.nn.Module):
    def __init__(self, input_size, hidden_size=512, d_ff=2048, num_heads=8, num_layers=6, bidirectional=False, cross_attention=False,
                 norm='layer', norm_first=True, activation_ff='relu', positional_encoding=True):
        super().__init__()
        self.positional_encoding = positional_encoding
        self.lin = torch.nn.Linear(input_size, hidden_size)
        self.transformer_layers = torch.nn.ModuleList([
            TransformerLayer(hidden_size, d_ff, num_heads, bidirectional, cross_attention, norm, norm_first, activation_ff)
            for _ in range(num_layers)])

    def forward(self, x, seq_len, m=None, seq_len_m=None, state=None):
        h = self.lin(x)
        if self.positional_encoding:
            h = h + positional_encoding(h.shape[1], h.shape[2])
        state = [None] * len(self.transformer_layers) if state is None else list(state)
        for i, layer in enumerate(self.transformer_layers):
            h, state[i] = layer(h, seq_len, m=m, seq_len_m=seq_len_m, state=state[i])
        return h, state


# ------------------------------------------------------------------------------------------------ the fixture's variants
BASE = dict(input_size=10, hidden_size=48, d_ff=40, num_heads=3, num_layers=2)


def variant_kwargs(cfg):
    return {**BASE, **{k: cfg[k] for k in ('bidirectional', 'cross_attention', 'norm', 'norm_first')}}


def variant_stack(cfg, cls=None):
    return (cls or TransformerLayerStack)(**variant_kwargs(cfg))


def state_dict_of(g, name):
    return {k: torch.from_numpy(g[f'{name}/p_{k}']) for k in g['variants'][name]['keys']}


def variant_inputs(g, name, dtype=torch.float64, device='cpu'):
    cfg = g['variants'][name]

    def t(key):
        return torch.from_numpy(g[f'{name}/{key}']).to(dtype).to(device)
    x = t('x').requires_grad_()
    m = t('m').requires_grad_() if cfg['cross_attention'] else None
    state = [t(f'state{i}') for i in range(BASE['num_layers'])] if cfg['state'] else None
    return cfg, x, m, state, t('w')


def run_variant(g, name):
    """The restatement's fp64 run: ``(y, states, grads)`` with ``grads`` keyed ``x``, ``m`` and the parameter names."""
    cfg, x, m, state, w = variant_inputs(g, name)
    net = variant_stack(cfg).double()
    net.load_state_dict(state_dict_of(g, name), strict=True)
    y, states = net(x, cfg['seq_len'], m=m, seq_len_m=cfg['seq_len_m'], state=state)
    (y * w).sum().backward()
    grads = {k: p.grad for k, p in net.named_parameters()}
    grads['x'] = x.grad
    if m is not None:
        grads['m'] = m.grad
    return y.detach(), [s.detach() for s in states], grads
