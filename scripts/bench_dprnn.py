#!/usr/bin/env python3
"""Time the dual-path RNN separator: forward + backward of ``DPRNN(64, 128, 100, 50, 6)`` at B = 4, L = 3999 frames (4 s at 8 kHz behind
a coder of window 16) and of its two chunk recurrences alone (intra: 324 sequences of 100 steps; inter: 400 sequences of 81 steps; one
bidirectional LSTM layer of 128 units, input projection and weight gradients included), on the HIP kernels (padertorch_amd.ops.dprnn +
the split-fp16 GEMM) and on the torch library path - a restatement with the same parameters on ``torch.nn.LSTM`` (MIOpen), ``F.linear``
and ``F.layer_norm`` with the reference's rearranges - on the same GPU in the same process.  The two recurrence kernels are also timed
without their GEMMs; per time step the whole layer is compared with the library's whole layer, and the kernels alone are listed apart.
The project's persistent recurrence (``ops.lstm.packed_lstm``) is run at the intra shape if it accepts it; a refusal is recorded.

    python scripts/bench_dprnn.py [--iters 10] [--warmup 3] [--rounds 5] [--out profiles/dprnn.txt]

Method (as scripts/bench_convnet.py): every chain is warmed up, then timed in ``rounds`` windows of ``iters`` iterations between two
events, the chains alternating window by window; reported are the median window (us per iteration) and min .. max.  Needs a GPU.
"""
import argparse
import json
import statistics
import sys
from pathlib import Path

import torch
import torch.nn.functional as F

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

B, L, N, H, K, P, BLOCKS = 4, 3999, 64, 128, 100, 50, 6


def library_chunk(chunk, x, intra):            # x [B, S, K, N]
    b, s, k, n = x.shape
    seqs = x.reshape(b * s, k, n) if intra else x.permute(0, 2, 1, 3).reshape(b * k, s, n)
    h = chunk.rnn(seqs)[0]
    z = F.layer_norm(F.linear(h, chunk.fc.weight, chunk.fc.bias), (n,), chunk.norm.weight, chunk.norm.bias, chunk.norm.eps)
    z = z.reshape(b, s, k, n) if intra else z.reshape(b, k, s, n).permute(0, 2, 1, 3)
    return z + x


def library_dprnn(net, x):
    from padertorch_amd.ops import dprnn
    S = dprnn.num_chunks(x.shape[1], K, P)
    pad = F.pad(x, [0, 0, K - P, (S - 1) * P + K - (x.shape[1] + K - P)])
    h = pad.unfold(1, K, P).permute(0, 1, 3, 2)
    for block in net.dprnn_blocks:
        h = library_chunk(block.inter_chunk_rnn, library_chunk(block.intra_chunk_rnn, h, True), False)
    out = x.new_zeros(x.shape[0], (S - 1) * P + K, x.shape[2])
    for s in range(S):
        out[:, s * P:s * P + K] += h[:, s]
    return out[:, K - P:-(K - P)]


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    from padertorch_amd.modules import DPRNN
    from padertorch_amd.ops import dprnn
    torch.manual_seed(0)
    net = DPRNN(N, H, K, P, BLOCKS).cuda()
    x = torch.randn(B, L, N, device='cuda', requires_grad=True)
    S = dprnn.num_chunks(L, K, P)
    rows = torch.randn(B * S * K, N, device='cuda', requires_grad=True)
    _, intra, inter = dprnn.tables(rows, None, B, S, K, P)
    rnn = net.dprnn_blocks[0].intra_chunk_rnn.rnn
    for p in rnn.parameters():
        p.requires_grad_(True)
    params = list(net.parameters())

    def step(fn, leaves):
        def run():
            y = fn()
            torch.autograd.grad(y, leaves, torch.ones_like(y))
        return run

    seg4 = rows.view(B, S, K, N)
    gates = torch.randn(B * S * K, 8 * H, device='cuda')
    dh = torch.randn(B * S * K, 2 * H, device='cuda')
    w = (rnn.weight_hh_l0.detach(), rnn.weight_hh_l0_reverse.detach())
    bias = (rnn.bias_hh_l0.detach(), rnn.bias_hh_l0_reverse.detach())

    def kernels(table, cap):
        def run():
            g = gates.clone()
            h, c = torch.ops.ptmi.chunk_lstm_forward(g, w[0], w[1], bias[0], bias[1], table, cap, H)
            torch.ops.ptmi.chunk_lstm_backward(g, dh, w[0], w[1], h, c, table, cap, H)
        return run

    chains = {
        'dprnn fwd+bwd, HIP': step(lambda: net(x), [x] + params),
        'dprnn fwd+bwd, library': step(lambda: library_dprnn(net, x), [x] + params),
        'intra LSTM layer fwd+bwd (324 x 100), HIP': step(lambda: dprnn.chunk_lstm(rows, intra, K, rnn), [rows] + list(rnn.parameters())),
        'intra LSTM layer fwd+bwd (324 x 100), library': step(lambda: rnn(seg4.reshape(B * S, K, N))[0], [rows] + list(rnn.parameters())),
        'inter LSTM layer fwd+bwd (400 x 81), HIP': step(lambda: dprnn.chunk_lstm(rows, inter, S, rnn), [rows] + list(rnn.parameters())),
        'inter LSTM layer fwd+bwd (400 x 81), library': step(lambda: rnn(seg4.permute(0, 2, 1, 3).reshape(B * K, S, N))[0],
                                                             [rows] + list(rnn.parameters())),
        'intra recurrence kernels fwd+bwd + one copy of the gates, HIP': kernels(intra, K),
        'inter recurrence kernels fwd+bwd + one copy of the gates, HIP': kernels(inter, S),
        'copy of the gates alone': lambda: gates.clone(),
    }
    # this project's persistent recurrence (ops.lstm.packed_lstm: few rows, many units, hand-offs between workgroups) at the intra shape,
    # if it accepts it: strict mode turns "leaves the HIP path" into an error, which is recorded instead of a time
    from torch.nn.utils.rnn import pack_padded_sequence
    from padertorch_amd import _lib
    from padertorch_amd.ops import lstm as persistent
    steps_of = torch.full((B * S,), K)

    def through_persistent():
        return persistent.packed_lstm(rnn, pack_padded_sequence(seg4.reshape(B * S, K, N), steps_of, batch_first=True)).data

    strict, _lib.STRICT = _lib.STRICT, True
    note = None
    try:
        y = through_persistent()
        torch.autograd.grad(y, [rows], torch.ones_like(y))
        chains['intra LSTM layer fwd+bwd (324 x 100), persistent kernels of ops.lstm'] = step(through_persistent,
                                                                                              [rows] + list(rnn.parameters()))
    except Exception as e:                                               # noqa: BLE001 (whatever the refusal is, it is the result)
        note = f'{type(e).__name__}: {e}'
    res = timed(chains, args.iters, args.warmup, args.rounds)
    _lib.STRICT = strict
    copy = res['copy of the gates alone']['median_us']
    for name, steps in (('intra', K), ('inter', S)):
        k = res[f'{name} recurrence kernels fwd+bwd + one copy of the gates, HIP']['median_us'] - copy
        hip = res[[n for n in res if n.startswith(name + ' LSTM layer') and n.endswith('HIP')][0]]['median_us']
        lib = res[[n for n in res if n.startswith(name + ' LSTM layer') and n.endswith('library')][0]]['median_us']
        res[f'{name}: us per time step, whole layer fwd+bwd (projection, recurrence, all gradients)'] = dict(hip=hip / steps, library=lib / steps)
        res[f'{name}: us per time step, the two HIP recurrence kernels alone'] = dict(hip=k / steps)
    if note is not None:
        res['persistent kernels of ops.lstm at the intra shape'] = dict(refused=note[:300])
    lines = [f'# scripts/bench_dprnn.py: B={B} L={L} DPRNN({N}, {H}, {K}, {P}, {BLOCKS}), S={S}; {torch.cuda.get_device_name(0)}; '
             f'iters={args.iters} rounds={args.rounds}; median window (us per iteration), min .. max']
    lines += [json.dumps({'name': k, **{a: (round(b, 2) if isinstance(b, float) else b) for a, b in v.items()}}) for k, v in res.items()]
    text = '\n'.join(lines) + '\n'
    print(text, end='')
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(text)


if __name__ == '__main__':
    main()
