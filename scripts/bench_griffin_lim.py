#!/usr/bin/env python3
"""Time one iteration of fast Griffin-Lim (``ops.griffin_lim.gl_iterations``: csrc/griffin_lim.hip, csrc/stft.hip) on its two update paths:

    fused      istft_kernel, gl_stft_update_kernel (the forward STFT with the update as its epilogue), gl_finish_kernel
    composed   istft_kernel, stft_fwd_kernel, gl_update_kernel, gl_finish_kernel

at the shapes

    baseline   a [64, 1000, 257], STFT(512, 128)                                   the BASELINE front end
    docstring  a [16, 400, 513],  STFT(1024, 256, window='hann', fading='half')    the reference docstring's geometry

    python scripts/bench_griffin_lim.py [--iters 100] [--warmup 2] [--rounds 7] [--out profiles/griffin_lim.txt]

Method: a window is ONE ``gl_iterations`` call of ``iters`` iterations (``atol = 0``, no polling, so all of them run) between two events,
its buffers allocated in front of the first event; after ``warmup`` windows per path the paths alternate window by window; reported
are the median window (us per iteration) and min .. max, on the same GPU in the same process.  ``algorithmic_bytes``: per bin and
iteration 36 B fused (P read by the inverse; x, a read; x, P written) or 64 B composed (plus the spectrum written and read again, and
P's second pass), plus 8 B per audio sample (written by the inverse, read by the forward).  ``share_of_hbm_peak`` is that over the whole
iteration's time (three or four launches, their gaps included - not a kernel's rate).  Needs a GPU.
"""
import argparse
import json
import statistics
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

HBM_GBS = 8000.     # MI355X peak HBM bandwidth, GB/s
SHAPES = {
    'baseline': dict(rows=64, frames=1000, stft=dict(size=512, shift=128)),
    'docstring': dict(rows=16, frames=400, stft=dict(size=1024, shift=256, window='hann', fading='half')),
}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=100)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--rounds', type=int, default=7)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_griffin_lim.py needs an MI355X'
    assert args.iters >= 20, 'at least 20 iterations a window'
    from padertorch_amd.ops import STFT, griffin_lim as gl
    dev = torch.device('cuda:0')
    torch.manual_seed(20)
    lines = []
    for name, shape in SHAPES.items():
        st = STFT(**shape['stft'])
        samples = gl.round_trip_samples(st, shape['frames'])
        a = st(torch.randn(shape['rows'], samples, device=dev)).abs().contiguous()
        assert tuple(a.shape) == (shape['rows'], shape['frames'], st.size // 2 + 1), a.shape
        angle = torch.rand(a.shape, device=dev) * 6.2831853 - 3.1415927
        x0 = torch.ops.ptmi.gl_project(a, torch.stack((angle.cos(), angle.sin()), -1))

        def window(path):
            x, P = x0.clone(), x0.clone()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            info = gl.gl_iterations(a, x, P, st, 0.95, args.iters, 0., path=path, poll=0)
            e1.record()
            torch.cuda.synchronize()
            assert int(info.num_iterations) == args.iters
            return e0.elapsed_time(e1) * 1e3 / args.iters, info

        finals = {}
        for path in ('fused', 'composed'):
            for _ in range(args.warmup):
                _, finals[path] = window(path)
        worst = float(((finals['fused'].rmse - finals['composed'].rmse).abs() / finals['composed'].rmse).max())
        times = {'fused': [], 'composed': []}
        for _ in range(args.rounds):
            for path in times:
                times[path].append(window(path)[0])
        bins, audio = a.numel(), shape['rows'] * samples
        res = dict(what=f'{name}: a {list(a.shape)}, STFT{tuple(shape["stft"].values())}, {samples} samples a row, us per iteration')
        for path, per_bin in (('fused', 36), ('composed', 64)):
            t = times[path]
            nbytes = per_bin * bins + 8 * audio
            gbs = nbytes / (statistics.median(t) * 1e-6) / 1e9
            res[path] = dict(median_us=round(statistics.median(t), 1), min_us=round(min(t), 1), max_us=round(max(t), 1),
                             algorithmic_bytes=nbytes, achieved_GBs=round(gbs, 1), share_of_hbm_peak=round(gbs / HBM_GBS, 4))
        res['composed_over_fused'] = round(res['composed']['median_us'] / res['fused']['median_us'], 3)
        res['fused_is_faster'] = res['fused']['median_us'] < res['composed']['median_us']
        res['rmse_histories_max_relative_difference'] = float(f'{worst:.2e}')
        print(json.dumps(res), flush=True)
        lines.append(json.dumps(res))
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
