#!/usr/bin/env python3
"""Time contrib/je's sequence half: forward + backward of ``GRU(torch.nn.GRU(256, H, 2, bidirectional=True))`` for H = 256 and 128 at B =
16 and 64, T = 500, ragged and full; the two GRU recurrence kernels alone (one bidirectional layer, full lengths) in microseconds per time
step; and the five poolings of ``contrib/je/modules/reduce.py`` at ``[32, 256, 1000]`` in both layouts (``[B, C, T]`` along the last axis,
``[B, T, C]`` along axis 1), forward + backward.  Every row is compared with the library formulation in the same process on the same GPU:
``torch.nn.GRU`` (MIOpen) behind ``pack_padded_sequence`` / ``pad_packed_sequence`` with the reference's two rearranges, and the
reference's mask-multiply-reduce for the poolings (restated below from ``reduce.py``).

    python scripts/bench_je_rnn.py [--iters 5] [--warmup 2] [--rounds 3] [--out profiles/je_rnn.txt]

Method (as scripts/bench_dprnn.py): every chain is warmed up, then timed in ``rounds`` windows of ``iters`` iterations between two
events, the chains alternating window by window; reported are the median window (us per iteration) and min .. max.  Needs a GPU.
"""
import argparse
import json
import statistics
import sys
from pathlib import Path

import torch
from torch.nn.utils.rnn import pack_padded_sequence, pad_packed_sequence

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

N, T, LAYERS = 256, 500, 2
POOL_SHAPE = (32, 256, 1000)


def ragged(B, T):
    """Descending lengths from ``T`` down to ``T / 4`` (the library's ``pack_padded_sequence`` wants them sorted)."""
    return [int(round(T - (T - T // 4) * b / max(B - 1, 1))) for b in range(B)]


def library_rnn(rnn, x, lengths):
    """``rnn.py:26-49`` of the reference for a ``torch.nn.GRU``."""
    x = x.transpose(1, 2)
    if lengths is not None:
        x = pack_padded_sequence(x, lengths, batch_first=True)
    x, _ = rnn(x)
    if lengths is not None:
        x = pad_packed_sequence(x, batch_first=True)[0]
    return x.transpose(1, 2)


def _mask(x, lengths, axis):
    shape = [1] * x.dim()
    shape[axis] = x.shape[axis]
    lens = lengths.view([-1] + [1] * (x.dim() - 1))
    return (torch.arange(x.shape[axis], device=x.device).view(shape) < lens).to(x.dtype)


def library_pool(mode, x, lengths, axis, alpha):
    """``reduce.py`` of the reference: a mask tensor, a multiply (or add of its logarithm), a reduction."""
    axis = axis % x.dim()
    if mode == 'last':
        xt = x if axis == 1 else x.transpose(1, axis)
        return xt[torch.arange(x.shape[0], device=x.device), lengths - 1]
    mask = _mask(x, lengths, axis)
    if mode == 'sum':
        return (x * mask).sum(axis)
    if mode == 'mean':
        return (x * mask).sum(axis) / (mask.sum(axis) + 1e-6)
    if mode == 'max':
        return (x + torch.log(mask)).max(axis)[0]
    x_ = alpha * x
    x_ = x_ * mask + torch.log(mask)
    return (torch.softmax(x_, -1) * x).sum(-1)


def timed(chains, iters, warmup, rounds):
    for fn in chains.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    windows = {k: [] for k in chains}
    for _ in range(rounds):
        for k, fn in chains.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(iters):
                fn()
            e1.record()
            e1.synchronize()
            windows[k].append(e0.elapsed_time(e1) * 1e3 / iters)
    return {k: dict(median_us=statistics.median(v), min_us=min(v), max_us=max(v)) for k, v in windows.items()}


def step(fn, leaves):
    def run():
        y = fn()
        torch.autograd.grad(y, leaves, torch.ones_like(y))
    return run


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    from padertorch_amd import _lib
    from padertorch_amd.contrib.je.modules import GRU
    from padertorch_amd.ops import gru as ops_gru
    from padertorch_amd.ops.seq_pool import seq_pool
    torch.manual_seed(0)
    tile = int(_lib.load().ptmi_chunk_gru_tile())
    chains, per_step = {}, []
    for H in (256, 128):
        rnn = torch.nn.GRU(N, H, LAYERS, batch_first=True, bidirectional=True).cuda()
        net = GRU(rnn)
        params = list(rnn.parameters())
        for B in (16, 64):
            x = torch.randn(B, N, T, device='cuda', requires_grad=True)
            for tag, lengths in (('ragged', ragged(B, T)), ('full', None)):
                name = f'GRU 2 x bidirectional H={H} B={B} T={T} {tag} fwd+bwd'
                device_lengths = None if lengths is None else torch.tensor(lengths, device='cuda')
                chains[name + ', HIP'] = step(lambda net=net, x=x, n=device_lengths: net(x, n)[0], [x] + params)
                chains[name + ', library'] = step(lambda rnn=rnn, x=x, n=lengths: library_rnn(rnn, x, n), [x] + params)
            # one bidirectional layer's recurrence kernels alone, full lengths
            gates = torch.randn(B * T, 6 * H, device='cuda')
            dh = torch.randn(B * T, 2 * H, device='cuda')
            table = ops_gru.sequence_table(gates, None, B, T)
            w = (rnn.weight_hh_l0.detach(), rnn.weight_hh_l0_reverse.detach())
            b = (rnn.bias_hh_l0.detach(), rnn.bias_hh_l0_reverse.detach())

            def kernels(gates=gates, dh=dh, table=table, w=w, b=b, H=H):
                g = gates.clone()
                h, q = torch.ops.ptmi.chunk_gru_forward(g, w[0], w[1], b[0], b[1], table, T, H, False)
                torch.ops.ptmi.chunk_gru_backward(g, q, dh, w[0], w[1], h, table, T, H, False)

            def forward_only(gates=gates, table=table, w=w, b=b, H=H):
                torch.ops.ptmi.chunk_gru_forward(gates.clone(), w[0], w[1], b[0], b[1], table, T, H, False)

            key = f'H={H} B={B}'
            chains[f'recurrence kernels fwd+bwd + one copy of the gates, {key}'] = kernels
            chains[f'recurrence kernel fwd + one copy of the gates, {key}'] = forward_only
            chains[f'copy of the gates alone, {key}'] = lambda gates=gates: gates.clone()
            per_step.append(key)
    Bp, Cp, Tp = POOL_SHAPE
    lengths = torch.tensor(ragged(Bp, Tp), device='cuda')
    alpha = torch.nn.Parameter(torch.ones(Cp, 1, device='cuda'))
    for layout, shape, axis in (('[B, C, T] axis -1', (Bp, Cp, Tp), -1), ('[B, T, C] axis 1', (Bp, Tp, Cp), 1)):
        x = torch.randn(*shape, device='cuda', requires_grad=True)
        for mode in ('sum', 'mean', 'max', 'last', 'autopool'):
            xm, ax, leaves, a = x, axis, [x], None
            if mode == 'autopool':                      # [B, C, T] along the last axis: the second layout is its transposed view
                xm, ax, leaves, a = (x if axis == -1 else x.transpose(1, 2)), -1, [x, alpha], alpha
            name = f'{mode} {layout} {list(POOL_SHAPE)} ragged fwd+bwd'

            def hip(xm=xm, ax=ax, mode=mode, a=a):
                y = seq_pool(xm, lengths, ax, mode, False, alpha=a)
                return y[0] if mode == 'max' else y

            chains[name + ', HIP'] = step(hip, leaves)
            chains[name + ', library'] = step(lambda xm=xm, ax=ax, mode=mode, a=a: library_pool(mode, xm, lengths, ax, a), leaves)
    res = timed(chains, args.iters, args.warmup, args.rounds)
    for key in per_step:
        copy = res[f'copy of the gates alone, {key}']['median_us']
        both = res[f'recurrence kernels fwd+bwd + one copy of the gates, {key}']['median_us'] - copy
        fwd = res[f'recurrence kernel fwd + one copy of the gates, {key}']['median_us'] - copy
        res[f'us per time step, one bidirectional layer, {key}, T={T} full, tile of {tile}'] = dict(
            forward_kernel=fwd / T, backward_kernel=(both - fwd) / T)
    for name in [n for n in res if n.endswith(', HIP')]:
        lib = name[:-len('HIP')] + 'library'
        res[name]['library_over_hip'] = res[lib]['median_us'] / res[name]['median_us']
    lines = [f'# scripts/bench_je_rnn.py: N={N} T={T} layers={LAYERS}, sequences per workgroup (tile) = {tile}; {torch.cuda.get_device_name(0)}; '
             f'iters={args.iters} rounds={args.rounds}; median window (us per iteration), min .. max; library_over_hip > 1: the HIP path is faster']
    lines += [json.dumps({'name': k, **{a: (round(b, 2) if isinstance(b, float) else b) for a, b in v.items()}}) for k, v in res.items()]
    text = '\n'.join(lines) + '\n'
    print(text, end='')
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(text)


if __name__ == '__main__':
    main()
