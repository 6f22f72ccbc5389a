#!/usr/bin/env python3
"""Time the three beamforming kernels (``ops.beamforming``: csrc/beamform.hip) at a CHiME-like shape: C = 6 channels, F = 513 bins
(``STFT(1024, 256)``), T = 600 frames, B in {1, 16} examples:

  * ``bf_psd``     both PSD matrices from one pass over the observation and the two ``[B, C, T, F]`` masks (channel medians in the
                   kernel), its partial-sum stage included;
  * ``bf_souden``  the solve per bin and the reference-channel stage (``ref_channel=None``);
  * ``bf_apply``   the vector applied to the observation;
  * ``mask_beamforming``  the three together, as ``SimpleMaskEstimator.enhance`` calls them;
  * ``bf_eig gev+ban`` / ``bf_eig pca``  the eigen launch alone, ``bf_phase`` the phase correction alone, and
    ``mask_beamforming gev+ban`` / ``mask_beamforming pca`` the chains beside the Souden chain of the same run; ``sweeps``: how many
    bins took how many Jacobi sweeps.  The eigen and phase kernels are latency-bound fp64 on ``B F`` bins: times only.

For every other entry: the time per call and the algorithmic bytes (what the operation has to read and write once: inputs and outputs, no
workspace) over that time, as GB/s and as a fraction of the MI355X's 8 TB/s peak HBM bandwidth (a streaming copy reaches about 0.79
of it).

    python scripts/bench_beamforming.py [--reps 20] [--warmup 3] [--rounds 7] [--out profiles/beamforming.txt]

Method: ``reps`` calls are captured into one graph, so that the host's launch cost (more than a B = 1 kernel takes) is not in the
window; every call of a graph reads ANOTHER copy of the inputs, enough copies that a replay moves more than twice the 256 MB
Infinity Cache, so the bytes come from HBM.  Each graph is warmed up and replayed ``rounds`` times between two events; reported are the
median replay (us per call) and min .. max.  Needs a GPU.
"""
import argparse
import json
import statistics
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

C, T, F = 6, 600, 513
HBM_GBS = 8000.         # MI355X peak HBM bandwidth, GB/s
CACHE_BYTES = 256e6     # Infinity Cache


def graph_of(fn, reps):
    """``fn(i)`` for ``i < reps`` as one graph (warmed up eagerly on the capture stream first)."""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fn(0)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        keep = [fn(i) for i in range(reps)]
    return graph, keep


def replay_us(graph, reps):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    graph.replay()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) * 1e3 / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_beamforming.py needs an MI355X'
    from padertorch_amd import ops  # noqa: F401  (registers torch.ops.ptmi.*)
    dev = torch.device('cuda:0')
    torch.manual_seed(0)
    lines = []
    for B in (1, 16):
        n = B * C * T * F
        in_bytes = n * 8 + 2 * n * 4                                     # the observation and two masks
        copies = min(args.reps, max(1, int(2 * CACHE_BYTES // in_bytes) + 1))
        Y = [torch.randn(B, C, T, F, dtype=torch.complex64, device=dev) for _ in range(copies)]
        speech = [torch.rand(B, C, T, F, device=dev) for _ in range(copies)]
        noise = [1 - s for s in speech]
        psd = [torch.ops.ptmi.bf_psd(Y[i], speech[i], noise[i], None, True) for i in range(copies)]
        w = [torch.ops.ptmi.bf_souden(p[0], p[1], -1)[0] for p in psd]
        psd_bytes = 2 * B * F * C * C * 16
        series = {
            'bf_psd': (lambda i: torch.ops.ptmi.bf_psd(Y[i % copies], speech[i % copies], noise[i % copies], None, True),
                       in_bytes + psd_bytes),
            'bf_souden': (lambda i: torch.ops.ptmi.bf_souden(psd[i % copies][0], psd[i % copies][1], -1),
                          psd_bytes + B * F * C * C * 8 + 2 * B * F * C * 16 + B * F * C * 8),
            'bf_apply': (lambda i: torch.ops.ptmi.bf_apply(w[i % copies], Y[i % copies], None), n * 8 + B * T * F * 8 + B * F * C * 8),
            'mask_beamforming': (lambda i: ops.mask_beamforming(Y[i % copies], speech[i % copies], noise[i % copies]),
                                 in_bytes + n * 8 + B * T * F * 8),
            # latency- and LDS-bound fp64 on B F bins (no bytes: a share of the HBM peak would say nothing about them)
            'bf_eig gev+ban': (lambda i: torch.ops.ptmi.bf_eig(psd[i % copies][0], psd[i % copies][1], True, True), None),
            'bf_eig pca': (lambda i: torch.ops.ptmi.bf_eig(psd[i % copies][0], None, False, False), None),
            'bf_phase': (lambda i: torch.ops.ptmi.bf_phase(w[i % copies]), None),
            'mask_beamforming gev+ban': (lambda i: ops.mask_beamforming(Y[i % copies], speech[i % copies], noise[i % copies],
                                                                        beamformer='gev+ban'), in_bytes + n * 8 + B * T * F * 8),
            'mask_beamforming pca': (lambda i: ops.mask_beamforming(Y[i % copies], speech[i % copies], noise[i % copies],
                                                                    beamformer='pca'), in_bytes + n * 8 + B * T * F * 8),
        }
        graphs = {k: graph_of(fn, args.reps) for k, (fn, _) in series.items()}
        for graph, _ in graphs.values():
            for _ in range(args.warmup):
                graph.replay()
        torch.cuda.synchronize()
        times = {k: [] for k in series}
        for _ in range(args.rounds):                                      # the series alternate round by round
            for k, (graph, _) in graphs.items():
                times[k].append(replay_us(graph, args.reps))
        res = dict(what=f'beamforming kernels, B={B} C={C} T={T} F={F}, {args.reps} calls per graph replay over {copies} input copies '
                        f'({copies * in_bytes / 1e6:.0f} MB)')
        for k, (_, nbytes) in series.items():
            us = statistics.median(times[k])
            res[k] = dict(median_us=round(us, 2), min_us=round(min(times[k]), 2), max_us=round(max(times[k]), 2))
            if nbytes is not None:
                res[k].update(bytes=nbytes, gb_per_s=round(nbytes / us / 1e3, 1), hbm_fraction=round(nbytes / us / 1e3 / HBM_GBS, 4))
        for k, gev in (('gev', True), ('pca', False)):                    # the Jacobi sweeps the bins of the first input copy took
            sweeps = torch.ops.ptmi.bf_eig(psd[0][0], psd[0][1], gev, False)[2].flatten().tolist()
            res[f'sweeps {k}'] = {str(s): sweeps.count(s) for s in sorted(set(sweeps))}
        lines.append(json.dumps(res))
        print(lines[-1], flush=True)
        del graphs
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
