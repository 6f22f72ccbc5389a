#!/usr/bin/env python3
"""Time BigVGAN's anti-aliased activation (up-sampling x2, SnakeBeta, low-pass and decimation x2; csrc/anti_alias.hip) against the
unfused formulation in torch ops (tests/anti_alias_ref.py on the same GPU), forward and forward + backward, at

    [8, 256, 2048]   [8, 64, 16384]   [8, 16, 131072]          (4.2 M, 8.4 M, 16.8 M elements)

    python scripts/bench_anti_alias.py [--window 0.5] [--rounds 3] [--out FILE]

Method.  Three ways of running one call are timed between two device events, after a warm-up of every one at every shape:

    fused_graph   the HIP launches alone: ``calls`` calls captured in a graph, the graph replayed - no host time between the kernels;
                  this is the KERNEL time (forward: one launch; backward: aa_backward_kernel + the parameter-gradient finishing kernel)
    fused_eager   the public module (``Activation1d(SnakeBeta)``), called from Python as a user does
    unfused_eager the restatement's torch ops on CUDA tensors (index gather, conv_transpose1d, sin, conv1d ... and autograd's backward)

A window repeats its call until at least ``--window`` seconds of device time have gone by (the count is fixed from a calibration run);
the three alternate window by window for ``--rounds`` rounds; the median window is reported.  ``GBs`` is the algorithmic traffic -
8 B per element forward (x read, y written), 12 B more backward (dy, x read, dx written) - over the kernel time.

The instruction-count estimate (``valu_per_element``) is read off the ISA of the default specialisation (hipcc -S, the loop bodies of
aa_forward_kernel<true, 4> / aa_backward_kernel<true, 4>; not measured): with 256 CUs x 4 SIMDs x 16 lanes at 2.4 GHz the VALU issues
39.3 T lane-instructions a second, HBM moves 8 TB/s; the smaller of the two element rates names the bound.  Needs a GPU.
"""
import argparse
import json
import statistics
import sys
from pathlib import Path

import torch

REPO = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(REPO), str(REPO / 'tests')]

HBM_GBS = 8000.                      # MI355X peak HBM bandwidth, GB/s
VALU_LANE_OPS = 256 * 4 * 16 * 2.4e9   # lane-instructions per second
#: VALU instructions per output element, from the ISA: forward 2 points x ~57 (6 FMAs, index arithmetic, sincos) + ~17 for the 12-tap
#: output; backward 2 points x ~118 (up-sampling, 6-tap adjoint, sincos, gradient terms, fp64 partials) + ~20 for the 12-tap dx gather
VALU_PER_ELEMENT = {'forward': 131, 'backward': 256}
SHAPES = [(8, 256, 2048), (8, 64, 16384), (8, 16, 131072)]
GRAPH_CALLS = 10


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e-3 / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--window', type=float, default=0.5, help='least device time of a window, seconds')
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_anti_alias.py needs an MI355X'
    import anti_alias_ref as ref
    from padertorch_amd.contrib.mk.synthesis.vocoder.nvidia_bigvgan import Activation1d, SnakeBeta
    dev = torch.device('cuda:0')
    torch.manual_seed(21)
    lines = []
    for shape in SHAPES:
        B, C, T = shape
        m = Activation1d(SnakeBeta(C, alpha_logscale=True)).to(dev)
        with torch.no_grad():
            m.act.alpha.normal_(0, 0.5)
            m.act.beta.normal_(0, 0.5)
        alpha, beta = m.act.alpha, m.act.beta
        up, down = m.upsample.filter.reshape(-1).contiguous(), m.downsample.lowpass.filter.reshape(-1).contiguous()
        x = torch.randn(shape, device=dev, requires_grad=True)
        w = torch.randn(shape, device=dev)
        xd, ad, bd = x.detach(), alpha.detach(), beta.detach()

        def fused_forward_op():
            return torch.ops.ptmi.anti_alias_forward(xd, up, down, ad, bd, 2, 2, True, True)

        def fused_backward_op():
            return torch.ops.ptmi.anti_alias_backward(w, xd, up, down, ad, bd, 2, 2, True, True, 2)

        def graph_of(fn):
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                fn()
            torch.cuda.current_stream().wait_stream(side)
            torch.cuda.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                for _ in range(GRAPH_CALLS):
                    keep = fn()
            graph.keep = keep
            return graph

        def module_forward():
            with torch.no_grad():
                return m(xd)

        def module_both():
            return torch.autograd.grad((m(x) * w).sum(), [x, alpha, beta])

        def unfused_forward():
            with torch.no_grad():
                return ref.activation1d(xd, ad, bd, up, down, 2, 2, True)

        def unfused_both():
            return torch.autograd.grad((ref.activation1d(x, alpha, beta, up, down, 2, 2, True) * w).sum(), [x, alpha, beta])

        res = dict(shape=list(shape), elements=B * C * T)
        # the two formulations agree (fp32 against fp32; the tests hold the gates against fp64)
        y_f, y_u = module_forward(), unfused_forward()
        res['max_abs_difference_fused_unfused'] = float(f'{float((y_f - y_u).abs().max()):.3g}')
        g_f, g_u = module_both(), unfused_both()
        res['max_rel_difference_dx'] = float(f'{float((g_f[0] - g_u[0]).abs().max() / g_u[0].abs().max()):.3g}')
        for mode, nbytes, graph_fns, eager, unfused in (
                ('forward', 8, (fused_forward_op,), module_forward, unfused_forward),
                ('forward_backward', 20, (fused_forward_op, fused_backward_op), module_both, unfused_both)):
            graphs = [graph_of(fn) for fn in graph_fns]

            def replay():
                for g in graphs:
                    g.replay()
            runs = {'fused_graph': (replay, GRAPH_CALLS), 'fused_eager': (eager, 1), 'unfused_eager': (unfused, 1)}
            reps, times = {}, {k: [] for k in runs}
            for name, (fn, calls) in runs.items():                 # warm-up and calibration
                timed(fn, 3)
                per = timed(fn, 20)
                reps[name] = max(3, int(1.1 * args.window / per) + 1)
            for _ in range(args.rounds):
                for name, (fn, calls) in runs.items():
                    t = timed(fn, reps[name])
                    while t * reps[name] < args.window:             # a window shorter than asked for does not count
                        reps[name] = int(1.2 * reps[name] * args.window / (t * reps[name])) + 1
                        t = timed(fn, reps[name])
                    times[name].append(t / calls)
            out = {}
            for name, t in times.items():
                med = statistics.median(t)
                out[name] = dict(median_us=round(med * 1e6, 2), min_us=round(min(t) * 1e6, 2), max_us=round(max(t) * 1e6, 2),
                                 calls_in_last_window=reps[name] * runs[name][1], least_window_s=round(min(t) * reps[name] * runs[name][1], 3))
            kernel = out['fused_graph']['median_us'] * 1e-6
            out['algorithmic_bytes'] = nbytes * B * C * T
            out['kernel_GBs'] = round(nbytes * B * C * T / kernel / 1e9, 1)
            out['share_of_hbm_peak'] = round(out['kernel_GBs'] / HBM_GBS, 4)
            valu = VALU_PER_ELEMENT['forward'] + (VALU_PER_ELEMENT['backward'] if mode == 'forward_backward' else 0)
            valu_floor, hbm_floor = B * C * T * valu / VALU_LANE_OPS, nbytes * B * C * T / (HBM_GBS * 1e9)
            out['estimate_not_measured'] = dict(valu_per_element=valu, valu_issue_floor_us=round(valu_floor * 1e6, 2),
                                                hbm_floor_us=round(hbm_floor * 1e6, 2),
                                                bound='VALU issue' if valu_floor > hbm_floor else 'HBM',
                                                kernel_over_larger_floor=round(kernel / max(valu_floor, hbm_floor), 2))
            out['unfused_over_fused_eager'] = round(out['unfused_eager']['median_us'] / out['fused_eager']['median_us'], 2)
            out['unfused_over_fused_kernel'] = round(out['unfused_eager']['median_us'] / out['fused_graph']['median_us'], 2)
            res[mode] = out
        print(json.dumps(res), flush=True)
        lines.append(json.dumps(res))
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
