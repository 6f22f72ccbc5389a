#!/usr/bin/env python3
"""Time contrib/je's convolution stack: forward and forward + backward of a ``CNN1d``, eagerly and as a replayed ``torch.cuda.graph``, at
``B = 16``, ``T = 1000`` for

    wide        CNN1d(256, [256] * 3, 3, norm='batch')
    wide gated  the same with gated=True
    narrow      CNN1d(64, [64] * 3, 5, norm='batch')

and one block of each alone (``Conv1d(C, C, K, norm='batch'[, gated=True])``: the per-block split).  Every row is compared with the library
composition on the same GPU in the same process, built from the SAME parameters: ``F.pad``, ``F.conv1d`` (MIOpen), this package's
``Normalization``, the torch activation, the sigmoid gate.  No lengths (a graph needs none); statistics over the whole batch.

    python scripts/bench_je_conv.py [--iters 10] [--warmup 3] [--rounds 5] [--out profiles/je_conv.txt]

Method (as scripts/bench_je_rnn.py): every chain is warmed up, then timed in ``rounds`` windows of ``iters`` iterations between two events,
the chains alternating window by window; reported are the median window (us per iteration) and min .. max.  Needs a GPU.
"""
import argparse
import statistics
import sys
from pathlib import Path

import torch
import torch.nn.functional as F

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

B, T = 16, 1000
GEOMETRIES = {'wide': (256, 3, False), 'wide gated': (256, 3, True), 'narrow': (64, 5, False)}


def library_block(m, x):
    """One ``Conv1d`` block of the reference's formulation on library kernels, with the module's own parameters."""
    from padertorch_amd.contrib.je.modules.conv_utils import compute_pad_size
    xp = F.pad(x, compute_pad_size(m.kernel_size, m.dilation, m.stride, m.pad_type))
    y = F.conv1d(xp, m.conv.weight, m.conv.bias, stride=m.stride, dilation=m.dilation)
    if m.norm is not None:
        y = m.norm(y)
    y = m.activation_fn(y)
    if m.gated:
        y = y * torch.sigmoid(F.conv1d(xp, m.gate_conv.weight, m.gate_conv.bias, stride=m.stride, dilation=m.dilation))
    return y


def library_cnn(net, x):
    for conv in net.convs:
        x = library_block(conv, x)
    return x


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
    return {k: (statistics.median(v), min(v), max(v)) for k, v in windows.items()}


def chain(fn, x, params, backward):
    def run():
        y = fn(x)
        if backward:
            torch.autograd.grad(y.sum(), [x] + params)
        return y
    return run


def graphed(run):
    """``run`` as a replayed graph (captured on a side stream after a warm-up there)."""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            run()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        run()
    return graph.replay


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    from padertorch_amd.contrib.je.modules import CNN1d
    lines = [f'contrib/je CNN1d, B = {B}, T = {T}, norm = batch, fp32; us per iteration: median (min .. max) of {args.rounds} windows of '
             f'{args.iters}; ratio = library / ours (above 1: ours is faster)', torch.cuda.get_device_name(0), '']
    for name, (C, K, gated) in GEOMETRIES.items():
        torch.manual_seed(0)
        net = CNN1d(C, [C] * 3, K, norm='batch', gated=gated).cuda()
        x = torch.randn(B, C, T, device='cuda', requires_grad=True)
        params = list(net.parameters())
        subjects = {'stack': (lambda v: net(v)[0], lambda v: library_cnn(net, v), params),
                    'block': (lambda v: net.convs[1](v)[0], lambda v: library_block(net.convs[1], v), list(net.convs[1].parameters()))}
        for what, (ours, lib, ps) in subjects.items():
            for backward in (False, True):
                eager = {'ours': chain(ours, x, ps, backward), 'library': chain(lib, x, ps, backward)}
                chains = dict(eager)
                for k, fn in eager.items():
                    chains[k + ' graph'] = graphed(fn)
                res = timed(chains, args.iters, args.warmup, args.rounds)
                for mode in ('', ' graph'):
                    a, b = res['ours' + mode], res['library' + mode]
                    # (an eager iteration carries the host's launch work, a replay does not: the two modes are separate comparisons)
                    lines.append(f'{name:11s} {what:5s} {"fwd+bwd" if backward else "fwd    "} {"graph" if mode else "eager"}  '
                                 f'ours {a[0]:8.1f} ({a[1]:8.1f} .. {a[2]:8.1f})   library {b[0]:8.1f} ({b[1]:8.1f} .. {b[2]:8.1f})   '
                                 f'ratio {b[0] / a[0]:5.2f}')
                print(lines[-2], lines[-1], sep='\n', flush=True)
    text = '\n'.join(lines) + '\n'
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(text)
    print(text)


if __name__ == '__main__':
    main()
