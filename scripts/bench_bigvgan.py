#!/usr/bin/env python3
"""Time the BigVGAN generator (csrc/bigvgan.hip, ops/bigvgan.py, contrib/mk/synthesis/vocoder/nvidia_bigvgan/bigvgan.py) beside the same
generator with torch's own convolutions on the same GPU.

    python scripts/bench_bigvgan.py [--frames 100 400] [--window 0.2] [--rounds 3] [--out profiles/bigvgan.txt]

Net: the geometry of bigvgan_v2_24khz_100band_256x with seeded weights (no checkpoint is needed): 100 mel bands, 1536 initial channels,
rates (4,4,2,2,2,2) / kernels (8,8,4,4,4,4), blocks (3,7,11) x (1,3,5), AMPBlock1, snakebeta log-scale, no tanh, no final bias.  B = 1.

    generator   the whole forward, eager and as a replayed ``torch.cuda.graph``: ours with the automatic path choice (``DIRECT_UP_TO``),
                with every convolution on the GEMM path, with the direct kernel wherever it is allowed - and ``library``: the same modules'
                ``Activation1d`` launches around ``torch.nn.functional.conv1d`` / ``conv_transpose1d`` (MIOpen), residual adds and the block
                mean as torch operators.  Alternating windows of at least ``--window`` seconds between device events, median of ``--rounds``.
    stages      device events between conv_pre, every stage's up-sampler and blocks, and the tail, eager, ours (automatic) and library.
    convolutions  every distinct Conv1d of the net (and a few widths between) on both paths, eager, measured first: the crossover table
                ``ops.bigvgan.DIRECT_UP_TO`` is derived from these rows (the line ``DIRECT_UP_TO``), and ``hip_auto`` runs with it.
Recorded, not gated.  One JSON line per measurement.  Needs a GPU.
"""
import argparse
import datetime
import json
import platform
import statistics
import sys
from pathlib import Path

import torch
import torch.nn.functional as F

REPO = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(REPO)]

H = dict(num_mels=100, upsample_initial_channel=1536, upsample_rates=[4, 4, 2, 2, 2, 2], upsample_kernel_sizes=[8, 8, 4, 4, 4, 4],
         resblock='1', resblock_kernel_sizes=[3, 7, 11], resblock_dilation_sizes=[[1, 3, 5], [1, 3, 5], [1, 3, 5]],
         activation='snakebeta', snake_logscale=True, use_tanh_at_final=False, use_bias_at_final=False, sampling_rate=24000)


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e-3 / reps


def windows(runs, window, rounds):
    """Median / min / max seconds per call of every entry of ``runs``, the entries alternating within a round."""
    reps, times = {}, {k: [] for k in runs}
    for name, fn in runs.items():
        timed(fn, 2)
        reps[name] = max(2, int(1.1 * window / max(timed(fn, 2), 1e-7)) + 1)
    for _ in range(rounds):
        for name, fn in runs.items():
            times[name].append(timed(fn, reps[name]))
    return {k: dict(median_ms=round(statistics.median(t) * 1e3, 4), min_ms=round(min(t) * 1e3, 4), max_ms=round(max(t) * 1e3, 4),
                    calls_per_window=reps[k]) for k, t in times.items()}


def seeded_model(dev):
    from padertorch_amd.contrib.mk.synthesis.vocoder.nvidia_bigvgan import BigVGAN
    torch.manual_seed(23)
    m = BigVGAN(H)
    with torch.no_grad():
        for name, p in m.named_parameters():
            if name.endswith('.weight'):
                fan_in = (p.shape[0] if name.startswith('ups.') else p.shape[1]) * p.shape[2]
                p.copy_(torch.randn(p.shape) * fan_in ** -0.5)
            elif name.endswith('.bias'):
                p.copy_(0.1 * torch.randn(p.shape))
            else:
                p.copy_(0.3 * torch.randn(p.shape))
    return m.to(dev).eval()


def library_stages(m, x, mark=lambda name: None):
    """The generator with torch's convolutions; ``mark(name)`` is called behind every stage."""
    nk = m.num_kernels

    def conv(c, v):
        K = c.weight.shape[2]
        return F.conv1d(v, c.weight, c.bias, dilation=c.dilation, padding=(K - 1) * c.dilation // 2)
    x = conv(m.conv_pre, x)
    mark('conv_pre')
    for i in range(m.num_upsamples):
        up = m.ups[i][0]
        k = up.weight.shape[2]
        x = F.conv_transpose1d(x, up.weight, up.bias, stride=up.stride, padding=(k - up.stride) // 2)
        mark(f'up{i}')
        xs = None
        for j in range(nk):
            blk = m.resblocks[i * nk + j]
            v = x
            for c1, c2, a1, a2 in zip(blk.convs1, blk.convs2, blk.activations[::2], blk.activations[1::2]):
                v = conv(c2, a2(conv(c1, a1(v)))) + v
            xs = v if xs is None else xs + v
        x = xs / nk
        mark(f'blocks{i}')
    x = conv(m.conv_post, m.activation_post(x)).clamp(-1.0, 1.0)
    mark('post')
    return x


def our_stages(m, x, mark=lambda name: None):
    """``BigVGAN.forward`` step for step, with ``mark(name)`` behind every stage."""
    from padertorch_amd.ops import bigvgan as ops
    nk, path = m.num_kernels, m.conv_path
    x = m.conv_pre(x, path=path)
    mark('conv_pre')
    for i in range(m.num_upsamples):
        x = m.ups[i][0](x)
        mark(f'up{i}')
        xs = None
        for j in range(nk):
            xs = m.resblocks[i * nk + j](x, out=xs, scale=1.0 / nk, path=path)
        x = xs
        mark(f'blocks{i}')
    x = ops.conv_post(m.activation_post(x), m.conv_post.weight, m.conv_post.bias, tanh=m.use_tanh_at_final)
    mark('post')
    return x


def stage_times(fn, m, x, reps=5):
    names, rows = [], []
    for r in range(reps + 1):
        events, names = [torch.cuda.Event(enable_timing=True)], []
        events[0].record()

        def mark(name):
            ev = torch.cuda.Event(enable_timing=True)
            ev.record()
            events.append(ev)
            names.append(name)
        fn(m, x, mark)
        torch.cuda.synchronize()
        if r:                                               # (the first pass warms up)
            rows.append([a.elapsed_time(b) for a, b in zip(events, events[1:])])
    return {n: round(statistics.median(row[i] for row in rows), 4) for i, n in enumerate(names)}


def graphed(fn, x):
    """``fn(static_x)`` captured; returns (replay, static_y)."""
    static_x = x.clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fn(static_x)
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        static_y = fn(static_x)
    return g.replay, static_y


def derive_table(rows):
    """``DIRECT_UP_TO`` from the convolution rows: per K the widest C_in such that the direct kernel wins every row at that and at every
    narrower measured width."""
    table = {}
    for K in sorted({r['K'] for r in rows}):
        wins = {}
        for r in rows:
            if r['K'] == K and 'direct_us' in r:
                wins[r['C_in']] = wins.get(r['C_in'], True) and r['direct_us'] < r['gemm_us']
        best = 0
        for c in sorted(wins):
            if not wins[c]:
                break
            best = c
        table[K] = best
    full = {}
    for K in (1, 3, 5, 7, 9, 11):
        near = [table[k] for k in (K - 2, K, K + 2) if k in table] if K not in table else [table[K]]
        full[K] = min(near) if near else 0
    return full


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, nargs='+', default=[100, 400])
    ap.add_argument('--window', type=float, default=0.2, help='least device time of a generator window, seconds')
    ap.add_argument('--conv-window', type=float, default=0.02, help='least device time of a single-convolution window, seconds')
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_bigvgan.py needs an MI355X'
    from padertorch_amd.ops import bigvgan as ops
    dev = torch.device('cuda:0')
    lines = []

    def emit(res):
        print(json.dumps(res), flush=True)
        lines.append(json.dumps(res))

    emit(dict(what='box', device=torch.cuda.get_device_name(0), torch=torch.__version__, hip=torch.version.hip, host=platform.machine(),
              date=datetime.date.today().isoformat(), DIRECT_UP_TO=ops.DIRECT_UP_TO, DIRECT_MAX_CHANNELS=ops.DIRECT_MAX_CHANNELS, net=H))
    m = seeded_model(dev)
    total_up = 1
    for u in H['upsample_rates']:
        total_up *= u
    committed = dict(ops.DIRECT_UP_TO)
    wherever = {k: ops.DIRECT_MAX_CHANNELS for k in (1, 3, 5, 7, 9, 11)}

    def ours(x, table=None, path=None):
        saved = dict(ops.DIRECT_UP_TO)
        try:
            if table is not None:
                ops.DIRECT_UP_TO.clear()
                ops.DIRECT_UP_TO.update(table)
            m.conv_path = path
            return m(x)
        finally:
            m.conv_path = None
            ops.DIRECT_UP_TO.clear()
            ops.DIRECT_UP_TO.update(saved)

    with torch.no_grad():
        # -------------------------------------------------------------------- every convolution on both paths
        rows = []
        for T in args.frames:
            layers = [('conv_pre', H['num_mels'], H['upsample_initial_channel'], 7, 1, T)]
            t, ch = T, H['upsample_initial_channel']
            extra = {96: 128, 48: 64, 24: 32}
            for u in H['upsample_rates']:
                t, ch = t * u, ch // 2
                for c in (ch, extra.get(ch)):
                    if c is not None:
                        for K in H['resblock_kernel_sizes']:
                            for d in (1, 5):
                                layers.append((f'block {c}' + ('' if c == ch else ' (extra width)'), c, c, K, d, t))
            for name, c_in, c_out, K, d, t in layers:
                xx = torch.randn(1, c_in, t, device=dev)
                w = torch.randn(c_out, c_in, K, device=dev) * (c_in * K) ** -0.5
                b = torch.randn(c_out, device=dev) * 0.1
                r = torch.randn(1, c_out, t, device=dev)
                runs = {'gemm': lambda: ops.conv1d(xx, w, b, d, residual=r, path='gemm'),
                        'library': lambda: F.conv1d(xx, w, b, dilation=d, padding=(K - 1) * d // 2) + r}
                if ops.direct_ok(c_in, K, d):
                    runs['direct'] = lambda: ops.conv1d(xx, w, b, d, residual=r, path='direct')
                tm = windows(runs, args.conv_window, args.rounds)
                row = dict(what='conv1d + residual', layer=name, frames=T, C_in=c_in, C_out=c_out, K=K, dilation=d, T=t,
                           **{k + '_us': round(v['median_ms'] * 1e3, 2) for k, v in tm.items()})
                if 'direct' in tm:
                    row['gemm_over_direct'] = round(tm['gemm']['median_ms'] / tm['direct']['median_ms'], 3)
                rows.append(row)
                emit(row)
        derived = derive_table(rows)
        emit(dict(what='DIRECT_UP_TO', derived_from_the_rows_above=derived, in_ops_bigvgan=committed, equal=derived == committed,
                  rule='per K the widest measured C_in up to which, at every narrower measured width too, the direct kernel is faster than '
                       'the GEMM path in every row (both dilations, every frame count); K = 1, 5, 9 take the smaller of their neighbours',
                  note='hip_auto below runs with the derived table'))
        for T in args.frames:
            x = torch.randn(1, H['num_mels'], T, device=dev)
            # ---------------------------------------------------------------- the whole generator
            variants = {'hip_auto': lambda v: ours(v, derived), 'hip_all_gemm': lambda v: ours(v, path='gemm'),
                        'hip_direct_where_allowed': lambda v: ours(v, wherever), 'library': lambda v: library_stages(m, v)}
            y = {k: fn(x) for k, fn in variants.items()}
            scale = float(y['library'].abs().max())
            res = dict(what='generator', frames=T, samples=T * total_up, B=1,
                       max_abs_output=round(scale, 4),
                       max_difference_from_library={k: float(f'{float((v - y["library"]).abs().max()) / scale:.3g}') for k, v in y.items()
                                                    if k != 'library'})
            res['eager'] = windows({k: (lambda fn=fn: fn(x)) for k, fn in variants.items()}, args.window, args.rounds)
            replays = {}
            for k, fn in variants.items():
                replays[k], static_y = graphed(fn, x)
                replays[k]()
                torch.cuda.synchronize()
                if k != 'library':
                    assert torch.equal(static_y, y[k]), k     # the replay gives the eager call's bits
            res['graph_replay'] = windows(replays, args.window, args.rounds)
            for mode in ('eager', 'graph_replay'):
                res[f'library_over_hip_auto_{mode}'] = round(res[mode]['library']['median_ms'] / res[mode]['hip_auto']['median_ms'], 3)
            del replays
            emit(res)
            # ---------------------------------------------------------------- per stage
            saved = dict(ops.DIRECT_UP_TO)
            ops.DIRECT_UP_TO.update(derived)
            try:
                auto = stage_times(our_stages, m, x)
            finally:
                ops.DIRECT_UP_TO.update(saved)

            def all_gemm(mm, v, mark):
                mm.conv_path = 'gemm'
                try:
                    return our_stages(mm, v, mark)
                finally:
                    mm.conv_path = None
            emit(dict(what='stages (eager, ms)', frames=T, hip_auto=auto, library=stage_times(library_stages, m, x),
                      hip_all_gemm=stage_times(all_gemm, m, x)))
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
