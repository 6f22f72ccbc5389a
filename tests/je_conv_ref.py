"""An fp64 restatement in torch on the CPU, with autograd, of what the kernels of csrc/je_conv.hip compute for contrib/je's Conv1d, CNN1d
and Pool1d: the taps sum with padding, stride and dilation, the masked statistics, the epilogue and the pools.  It reads the geometry and
the parameters from the modules under test and shares no arithmetic with them.  tests/test_je_conv_host.py pins it to the reference's
fp64 run (tests/golden/g26_je_conv.npz)."""
import math

import numpy as np
import torch


def pad_size(kernel_size, dilation, stride, pad_type):
    span = 1 + dilation * (kernel_size - 1)
    if pad_type is None:
        return 0, 0
    if pad_type == 'front':
        return max(span - stride, 0), min(stride - 1, span - 1)
    if pad_type == 'both':
        return max(span - stride, 0) // 2, min(stride - 1, span - 1) + math.ceil(max(span - stride, 0) / 2)
    assert pad_type == 'end', pad_type
    return 0, span - 1


def out_size(n, kernel_size, dilation, stride, pad_type):
    return 1 + (n + sum(pad_size(kernel_size, dilation, stride, pad_type)) - 1 - dilation * (kernel_size - 1)) // stride


def padded(x, front, end):
    """``x [B, C, T]`` with ``front`` zeros before and ``end`` zeros behind the time axis."""
    B, C, _ = x.shape
    return torch.cat([x.new_zeros(B, C, front), x, x.new_zeros(B, C, end)], dim=2)


def taps(x, weight, bias, stride, dilation, front, end):
    """``z[b, co, t] = bias[co] + sum_k sum_ci weight[co, ci, k] xpad[b, ci, t stride + k dilation]``."""
    K = weight.shape[2]
    xp = padded(x, front, end)
    T_out = (xp.shape[2] - 1 - dilation * (K - 1)) // stride + 1
    z = x.new_zeros(x.shape[0], weight.shape[0], T_out)
    if bias is not None:
        z = z + bias[None, :, None]
    for k in range(K):
        z = z + torch.einsum('oc,bct->bot', weight[:, :, k], xp[:, :, k * dilation:k * dilation + (T_out - 1) * stride + 1:stride])
    return z


def mask_of(lengths, B, T):
    if lengths is None:
        return torch.ones(B, 1, T, dtype=torch.bool)
    return (torch.arange(T)[None, None, :] < torch.as_tensor(np.asarray(lengths))[:, None, None])


def masked_norm(x, lengths, kind, gamma, beta, eps, fixed=None):
    """``(y, mean, power, count)``: statistics over ``t < len_b`` ('batch': over b and t, 'sequence': per example), clamped variance,
    zero output behind the lengths (only when lengths are given).  ``fixed = (mean, rstd)`` replaces the measured statistics."""
    B, C, T = x.shape
    m = mask_of(lengths, B, T)
    xm = torch.where(m, x, torch.zeros_like(x))
    axes = (0, 2) if kind == 'batch' else (2,)
    n = m.to(x.dtype).expand(B, C, T).sum(axes, keepdim=True)
    mean = xm.sum(axes, keepdim=True) / n.clamp(min=1)
    power = (xm * xm).sum(axes, keepdim=True) / n.clamp(min=1)
    if fixed is None:
        rstd = 1 / torch.sqrt((power - mean * mean).clamp(min=0) + eps)
        y = (x - mean) * rstd
    else:
        y = (x - fixed[0]) * fixed[1]
    if gamma is not None:
        y = y * gamma.reshape(1, C, 1)
    if beta is not None:
        y = y + beta.reshape(1, C, 1)
    return torch.where(m, y, torch.zeros_like(y)), mean, power, n


def activation(x, fn):
    """``fn``: a torch activation module (its parameters in ``x``'s dtype)."""
    if isinstance(fn, torch.nn.PReLU):
        return torch.where(x < 0, fn.weight.to(x.dtype) * x, x)
    if isinstance(fn, torch.nn.LeakyReLU):
        return torch.where(x < 0, fn.negative_slope * x, x)
    if isinstance(fn, torch.nn.ELU):
        return torch.where(x > 0, x, fn.alpha * torch.expm1(x))
    if isinstance(fn, torch.nn.ReLU):
        return torch.where(x < 0, torch.zeros_like(x), x)
    if isinstance(fn, torch.nn.Tanh):
        return torch.tanh(x)
    if isinstance(fn, torch.nn.Sigmoid):
        return 1 / (1 + torch.exp(-x))
    assert isinstance(fn, torch.nn.Identity), fn
    return x


def _norm(norm, x, lengths, track):
    kind = 'batch' if norm.track_running_stats else 'sequence'
    fixed = None
    if norm.track_running_stats and not (norm.training and not norm.frozen_stats):
        fixed = (norm.running_mean, 1 / torch.sqrt(norm.running_var + norm.eps))
    y, mean, power, n = masked_norm(x, lengths, kind, norm.gamma, norm.beta, norm.eps, fixed)
    if track and fixed is None and norm.track_running_stats:
        with torch.no_grad():
            norm._update_running_stats(mean, power, n)
    return y


def pool(x, size, stride, pad_type, max_pool):
    """``(y, index)``: pad, trim the end to whole windows, pool; the indices count on the padded axis, the first of equal values wins."""
    front, end = pad_size(size, 1, stride, pad_type)
    xp = padded(x, front, end)
    xp = xp[..., :xp.shape[2] - max(xp.shape[2] - size, 0) % stride]
    win = xp.unfold(2, size, stride)                         # [B, C, T_out, size]
    if not max_pool:
        return win.mean(3), None
    first = (win == win.amax(3, keepdim=True)).to(torch.int64).argmax(3)
    return win.gather(3, first[..., None])[..., 0], first + torch.arange(win.shape[2]) * stride


def out_lengths(lengths, kernel_size, dilation, stride, pad_type):
    return None if lengths is None else np.asarray([out_size(int(n), kernel_size, dilation, stride, pad_type) for n in lengths])


def conv1d(m, x, lengths=None, residual=None, track=False):
    """The module ``m`` (a ``Conv1d`` in ``x``'s dtype on the CPU; only its attributes and parameters are read) on ``x [B, C, T]``."""
    front, end = pad_size(m.kernel_size, m.dilation, m.stride, m.pad_type)
    new_lengths = out_lengths(lengths, m.kernel_size, m.dilation, m.stride, m.pad_type)
    if m.pre_activation:
        if m.norm is not None:
            x = _norm(m.norm, x, lengths, track)
        x = activation(x, m.activation_fn)
    y = taps(x, m.conv.weight, m.conv.bias, m.stride, m.dilation, front, end)
    if not m.pre_activation:
        if m.norm is not None:
            y = _norm(m.norm, y, new_lengths, track)
        y = activation(y, m.activation_fn)
    if m.gated:
        y = y / (1 + torch.exp(-taps(x, m.gate_conv.weight, m.gate_conv.bias, m.stride, m.dilation, front, end)))
    if residual is not None:
        y = y + residual
    return y, new_lengths


def cnn1d(m, x, lengths=None, track=False):
    """The module ``m`` (a ``CNN1d``) on ``x``: ``(y, lengths, pool indices per layer)``."""
    skips, indices = [], []
    for i, conv in enumerate(m.convs):
        if i == 0 and m.input_norm is not None:
            x = activation(_norm(m.input_norm, x, lengths, track), m.input_activation_fn)
        skips.append(x if m.residual_connections[i] + m.dense_connections[i] else None)
        x, lengths = conv1d(conv, x, lengths, track=track)
        for src, x_ in enumerate(skips):
            if x_ is None:
                continue
            if m.strides[i] > 1:
                x_ = skips[src] = pool(x_, m.strides[i], m.strides[i], m.pad_types[i], False)[0]
            if i + 1 in m.dense_connections[src]:
                x = torch.cat((x, x_[..., :x.shape[2]]), dim=1)
        for src, x_ in enumerate(skips):
            if x_ is not None and i + 1 in m.residual_connections[src]:
                key = f'{src}->{i + 1}'
                if key in m.residual_skip_convs:
                    x_, _ = conv1d(m.residual_skip_convs[key], x_, track=track)
                x = x + x_
            dst = m.dense_connections[src] + m.residual_connections[src]
            if dst and max(dst) <= i + 1:
                skips[src] = None
        if i == m.num_layers - 1 and m.output_norm is not None:
            x = activation(_norm(m.output_norm, x, lengths, track), m.output_activation_fn)
        index = None
        if m.pool_sizes[i] > 1:
            x, index = pool(x, m.pool_sizes[i], m.pool_strides[i], m.pad_types[i], m.pool_types[i] == 'max')
            lengths = out_lengths(lengths, m.pool_sizes[i], 1, m.pool_strides[i], m.pad_types[i])
            for src, x_ in enumerate(skips):
                if x_ is not None:
                    skips[src] = pool(x_, m.pool_strides[i], m.pool_strides[i], m.pad_types[i], False)[0]
        indices.append(index)
    return x, lengths, indices
