#!/usr/bin/env python3
"""Time the TasNet learned-basis coders: encode -> masked decode -> sum(y r) -> backward, on the HIP kernels (padertorch_amd.ops.tas)
and on the torch library path (F.conv1d + relu, the broadcast multiply, F.conv_transpose1d), on the same GPU in the same process.

    python scripts/bench_tas_coders.py [--iters 200] [--warmup 20] [--rounds 5] [--out FILE]
    python scripts/bench_tas_coders.py --trace-only          # the HIP chain alone, a few iterations: run it under
                                                             # rocprofv3 --kernel-trace --stats -d DIR -- python scripts/bench_tas_coders.py --trace-only

Method: per configuration every chain is warmed up, then timed in ``rounds`` windows of ``iters`` iterations each between two
events; the chains alternate window by window (HIP, library, HIP, ...).  Reported: the median window (us per iteration) and the
spread (min .. max over the windows).  The library chain is timed in two such series (A and B): the difference of their medians is
its own run-to-run spread, the only margin the comparison allows.  Needs a GPU; there is no fallback.
"""
import argparse
import json
import statistics
import sys
from pathlib import Path

import torch
import torch.nn.functional as F

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

#: (B, T, L, N, stride, K): the reference's default TasNet configuration, its win2 and its convnet configuration
CONFIGS = [(4, 32000, 16, 64, 8, 2), (1, 32000, 2, 64, 1, 2), (4, 32000, 20, 256, 10, 2)]


def make(cfg, device):
    from padertorch_amd.contrib.examples.source_separation.tasnet import TasDecoder, TasEncoder
    B, T, L, N, stride, K = cfg
    torch.manual_seed(0)
    enc = TasEncoder(L, N, stride).to(device)
    dec = TasDecoder(L, N, stride).to(device)
    x = torch.randn(B, T, device=device, requires_grad=True)
    frames = enc(x)[0].shape[2]
    mask = torch.rand(K, B, N, frames, device=device, requires_grad=True)
    r = torch.randn(K, B, (frames - 1) * stride + L, device=device)
    leaves = [x, mask, enc.encoder_1d.weight, dec.decoder_1d.weight]

    def hip():
        w, _ = enc(x)
        return torch.autograd.grad((dec.masked(mask, w) * r).sum(), leaves)

    def library():
        h = L // 2
        xp = F.pad(x, (0, (h - T % h) % h))
        w = F.relu(F.conv1d(xp[:, None], enc.encoder_1d.weight, None, stride=stride))
        y = F.conv_transpose1d((mask * w[None]).flatten(0, 1), dec.decoder_1d.weight, None, stride=stride)[:, 0]
        return torch.autograd.grad((y.view(r.shape) * r).sum(), leaves)

    return hip, library


def window(fn, iters):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) * 1e3 / iters        # us per iteration


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=200)
    ap.add_argument('--warmup', type=int, default=20)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--trace-only', action='store_true')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_tas_coders.py needs an MI355X'
    device = torch.device('cuda:0')
    lines = []
    for cfg in CONFIGS:
        hip, library = make(cfg, device)
        if args.trace_only:
            for _ in range(5):
                hip()
            torch.cuda.synchronize()
            continue
        for a, b in zip(hip(), library()):               # the two chains compute the same thing
            assert (a - b).abs().max() <= 2e-4 * b.abs().max(), cfg
        series = {'hip': (hip, []), 'library_a': (library, []), 'library_b': (library, [])}
        for fn, _ in series.values():
            for _ in range(args.warmup):
                fn()
        torch.cuda.synchronize()
        for _ in range(args.rounds):
            for fn, times in series.values():
                times.append(window(fn, args.iters))
        res = {k: dict(median_us=round(statistics.median(t), 1), min_us=round(min(t), 1), max_us=round(max(t), 1))
               for k, (_, t) in series.items()}
        lib = min(res['library_a']['median_us'], res['library_b']['median_us'])
        margin = abs(res['library_a']['median_us'] - res['library_b']['median_us'])
        res.update(config=dict(zip('B T L N stride K'.split(), cfg)), library_spread_us=round(margin, 1),
                   hip_no_slower=res['hip']['median_us'] <= lib + margin)
        lines.append(json.dumps(res))
        print(lines[-1], flush=True)
    if args.out and lines:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
