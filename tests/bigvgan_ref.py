"""Restatement of the BigVGAN generator's convolutions and of the generator itself in plain tensor arithmetic, dtype-generic (meant for
fp64 on the CPU): the yardstick for shapes tests/golden/g23_bigvgan.npz does not hold.  Written from the definitions (include/ptmi.h,
"The BigVGAN generator's convolutions"), one shifted product per tap - not through torch's convolution operators:

    conv1d            y[b,co,t]  = bias[co] + sum_k sum_ci w[co,ci,k] x[b,ci,t + (k - (K-1)/2) d]       (x zero outside [0, T))
                      epilogue   v = scale (y + residual);  out = v  or  out + v
    conv_transpose1d  full[b,co,f u + kk] += sum_ci w[ci,co,kk] x[b,ci,f];  y = bias + full[p : p + (T-1) u - 2p + k],  p = (k - u) // 2
    conv_post         tanh or clamp to [-1, 1] of conv1d with one output channel
    fold_weight_norm  g v / |v|, the norm over every axis but 0
    generator         bigvgan.py's forward: conv_pre; per stage the up-sampler and the mean over its AMP blocks; activation_post; conv_post

The activations are tests/anti_alias_ref.py's.  ``rel_dev`` and ``gate`` are that module's, too.
"""
import json
from pathlib import Path

import numpy as np
import torch

import anti_alias_ref as aref
from anti_alias_ref import gate, rel_dev  # noqa: F401

GOLDEN = Path(__file__).resolve().parent / 'golden' / 'g23_bigvgan.npz'


def conv1d(x, w, bias=None, dilation=1, residual=None, out=None, scale=1.0):
    B, C_in, T = x.shape
    C_out, _, K = w.shape
    h = (K - 1) // 2 * dilation
    xp = torch.zeros((B, C_in, T + 2 * h), dtype=x.dtype)
    xp[..., h:h + T] = x
    y = torch.zeros((B, C_out, T), dtype=x.dtype)
    for k in range(K):
        y = y + torch.einsum('oi,bit->bot', w[:, :, k], xp[..., k * dilation:k * dilation + T])
    if bias is not None:
        y = y + bias.view(1, -1, 1)
    if residual is not None:
        y = y + residual
    y = scale * y
    return y if out is None else out + y


def conv_transpose1d(x, w, bias, stride):
    B, C_in, T = x.shape
    _, C_out, k = w.shape
    p = (k - stride) // 2
    full = torch.zeros((B, C_out, (T - 1) * stride + k), dtype=x.dtype)
    for kk in range(k):
        full[..., kk:kk + (T - 1) * stride + 1:stride] += torch.einsum('io,bit->bot', w[:, :, kk], x)
    y = full[..., p:p + (T - 1) * stride - 2 * p + k]
    return y if bias is None else y + bias.view(1, -1, 1)


def conv_post(x, w, bias=None, tanh=True):
    y = conv1d(x, w, bias)
    return torch.tanh(y) if tanh else y.clamp(-1.0, 1.0)


def fold_weight_norm(g, v):
    norm = v.pow(2).sum(dim=tuple(range(1, v.dim())), keepdim=True).sqrt()
    return g * v / norm


def generator(state, h, x, dtype=torch.float64):
    """``dict(y, pre, up<i>, mean<i>)`` of the generator with the (folded) ``state`` on ``x``, computed in ``dtype``."""
    s = {k: v.to(dtype) for k, v in state.items()}
    x = x.to(dtype)
    logscale = bool(h['snake_logscale'])
    beta = h['activation'] == 'snakebeta'

    def act(prefix, v):
        return aref.activation1d(v, s[prefix + '.act.alpha'], s[prefix + '.act.beta'] if beta else None, s[prefix + '.upsample.filter'],
                                 s[prefix + '.downsample.lowpass.filter'], logscale=logscale)

    def conv(prefix, v, dilation=1, residual=None):
        return conv1d(v, s[prefix + '.weight'], s.get(prefix + '.bias'), dilation, residual)

    def block(n, v, dilations):
        pre = f'resblocks.{n}'
        for j, d in enumerate(dilations):
            if h['resblock'] == '1':
                xt = conv(f'{pre}.convs1.{j}', act(f'{pre}.activations.{2 * j}', v), d)
                v = conv(f'{pre}.convs2.{j}', act(f'{pre}.activations.{2 * j + 1}', xt), 1, residual=v)
            else:
                v = conv(f'{pre}.convs.{j}', act(f'{pre}.activations.{j}', v), d, residual=v)
        return v

    got = {}
    nk = len(h['resblock_kernel_sizes'])
    x = got['pre'] = conv('conv_pre', x)
    for i, u in enumerate(h['upsample_rates']):
        x = got[f'up{i}'] = conv_transpose1d(x, s[f'ups.{i}.0.weight'], s[f'ups.{i}.0.bias'], u)
        xs = None
        for j in range(nk):
            b = block(i * nk + j, x, h['resblock_dilation_sizes'][j])
            xs = b if xs is None else xs + b
        x = got[f'mean{i}'] = xs / nk
    x = act('activation_post', x)
    got['y'] = conv_post(x, s['conv_post.weight'], s.get('conv_post.bias'), tanh=h.get('use_tanh_at_final', True))
    return got


_GOLDEN = None


def golden():
    """tests/golden/g23_bigvgan.npz (loaded once; ``cases`` decoded)."""
    global _GOLDEN
    if _GOLDEN is None:
        d = dict(np.load(GOLDEN, allow_pickle=False))
        d['cases'] = json.loads(str(d['cases']))
        _GOLDEN = d
    return _GOLDEN


def case_names():
    return list(golden()['cases'])


def state(name, which='sd'):
    """The state dict of a case as float32 tensors (``which='sd_wn'``: before ``remove_weight_norm()``; case ``k1`` only)."""
    g = golden()
    pool = g['pool']
    return {key: torch.from_numpy(pool[off:off + int(np.prod(shape))].reshape(shape).copy())
            for key, (off, shape) in g['cases'][name][which].items()}


def case(name):
    """``(meta, x, fp64 tensors by quantity, dev32 by quantity)`` of a golden case."""
    g = golden()
    meta = g['cases'][name]
    want = {q: torch.from_numpy(g[f'{name}_{q}']) for q in meta['quantities']}
    dev32 = {q: float(g[f'{name}_dev32_{q}']) for q in meta['quantities']}
    return meta, torch.from_numpy(g[f'{name}_x']), want, dev32
