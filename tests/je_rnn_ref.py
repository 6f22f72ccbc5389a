"""fp64 restatements (own code, torch on the CPU, differentiable by autograd) of what ``csrc/gru.hip`` and ``csrc/seq_pool.hip`` compute:
one GRU layer over a sequence table, a stack of such layers as ``contrib.je.modules.rnn.RNN`` runs them, ``reverse_sequence`` and the
five poolings.  ``tests/test_je_rnn_host.py`` pins them to the reference's own results in ``tests/golden/g25_je_rnn.npz``; the GPU tests
compare the kernels against them at the shapes the fixture does not cover.
"""
import numpy as np
import torch

F64 = torch.float64


def gru_layer(x, table, cap, dirs, flip=False):
    """``x [rows, N]`` fp64 -> ``h [rows, D H]``.  ``table``: rows ``(base, stride, count)``; ``dirs``: ``(w_ih, w_hh, b_ih, b_hh)`` per
    direction (biases may be None).  Sequence ``i`` has the steps ``base + t stride``, ``t < min(count, cap)``; direction 0 walks them
    forwards and direction 1 backwards, both the other way round with ``flip``.  Rows of no step are zero."""
    rows, H = x.shape[0], dirs[0][1].shape[1]
    blocks = []
    for d, (w_ih, w_hh, b_ih, b_hh) in enumerate(dirs):
        out = [torch.zeros(H, dtype=F64) for _ in range(rows)]
        for base, stride, count in table:
            count = max(0, min(int(count), cap))
            steps = [int(base) + t * int(stride) for t in range(count)]
            if bool(d) != bool(flip):
                steps = steps[::-1]
            h = torch.zeros(H, dtype=F64)
            for row in steps:
                gi = w_ih @ x[row] + (0 if b_ih is None else b_ih)
                gh = w_hh @ h + (0 if b_hh is None else b_hh)
                r = torch.sigmoid(gi[:H] + gh[:H])
                z = torch.sigmoid(gi[H:2 * H] + gh[H:2 * H])
                n = torch.tanh(gi[2 * H:] + r * gh[2 * H:])
                h = (1 - z) * n + z * h
                out[row] = h
        blocks.append(torch.stack(out))
    return torch.cat(blocks, 1)


def gru_stack(x, lengths, layers, reverse=False):
    """``RNN(torch.nn.GRU, reverse=reverse)``: ``x [B, F, T]`` -> ``[B, D H, T]``; ``layers``: a list of ``dirs`` (see :func:`gru_layer`)."""
    B, _, T = x.shape
    lengths = [T] * B if lengths is None else [int(n) for n in lengths]
    table = [(b * T, 1, lengths[b]) for b in range(B)]
    h = x.transpose(1, 2).reshape(B * T, -1)
    for dirs in layers:
        h = gru_layer(h, table, T, dirs, flip=reverse)
    return h.reshape(B, T, -1).transpose(1, 2)


def gru_layers_from_state(state, prefix, num_layers, bidirectional, bias):
    """``layers`` for :func:`gru_stack` from a ``torch.nn.GRU`` state dict (numpy or torch values) under ``prefix``."""
    def get(name):
        return torch.as_tensor(np.asarray(state[prefix + name]), dtype=F64)
    layers = []
    for k in range(num_layers):
        dirs = []
        for suffix in ('', '_reverse') if bidirectional else ('',):
            dirs.append((get(f'weight_ih_l{k}{suffix}'), get(f'weight_hh_l{k}{suffix}'),
                         get(f'bias_ih_l{k}{suffix}') if bias else None, get(f'bias_hh_l{k}{suffix}') if bias else None))
        layers.append(dirs)
    return layers


def reverse_sequence(x, lengths=None):
    """``x [B, T, F]``: ``out[b, t] = x[b, len_b - 1 - t]`` below the length, ``x[b, (len_b - 1 - t) mod T] * 0`` behind it."""
    B, T, _ = x.shape
    if lengths is None:
        return x.flip(1)
    rows = []
    for b in range(B):
        n = int(lengths[b])
        idx = torch.tensor([(n - 1 - t) % T for t in range(T)])
        mask = torch.tensor([1. if t < n else 0. for t in range(T)], dtype=x.dtype)[:, None]
        rows.append(x[b, idx] * mask)
    return torch.stack(rows)


def mean_denominator(n):
    """``float(len) + 1e-6f`` in float32, as ``reduce.py:42`` evaluates it."""
    return float(np.float32(n) + np.float32(1e-6))


def seq_pool(x, lengths, axis, mode, keepdims=False, alpha=None):
    """The pooling ``mode`` ('sum', 'mean', 'max', 'last', 'autopool') of ``x`` (batch on axis 0) over ``axis`` below ``lengths``.  ``max``
    returns ``(values, indices)``.  A position behind the length is never read (see ``ops.seq_pool`` on the reference's ``NaN * 0``)."""
    ax = axis + x.dim() if axis < 0 else axis
    T = x.shape[ax]
    outs, idxs = [], []
    for b in range(x.shape[0]):
        n = T if lengths is None else max(0, min(int(lengths[b]), T))
        xb = x[b].narrow(ax - 1, 0, n)
        shape = list(x[b].shape)
        del shape[ax - 1]
        if mode == 'sum':
            y = xb.sum(ax - 1)
        elif mode == 'mean':
            y = x[b].mean(ax - 1) if lengths is None else xb.sum(ax - 1) / mean_denominator(n)
        elif mode == 'max':
            if n == 0:
                y, i = torch.full(shape, -np.inf, dtype=x.dtype), torch.zeros(shape, dtype=torch.int64)
            else:
                y, i = xb.max(ax - 1)
            idxs.append(i)
        elif mode == 'last':
            y = x[b].select(ax - 1, n - 1 if n > 0 else T - 1)
        elif mode == 'autopool':
            a = alpha if not torch.is_tensor(alpha) else alpha.reshape(-1, 1)
            if n == 0:
                y = torch.full(shape, np.nan, dtype=x.dtype)
            else:
                y = (torch.softmax(a * xb, ax - 1) * xb).sum(ax - 1)
        else:
            raise ValueError(mode)
        outs.append(y)
    y = torch.stack(outs)
    if keepdims:
        y = y.unsqueeze(ax)
    if mode == 'max':
        i = torch.stack(idxs)
        return y, (i.unsqueeze(ax) if keepdims else i)
    return y
