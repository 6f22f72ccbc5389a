#!/usr/bin/env python3
"""Measure the transformer encoder stack at the reference's default shape (hidden_size 512, 8 heads of 64, d_ff 2048, 6 layers, B = 16,
T = 250 and 1000, bidirectional with ragged lengths T/2 .. T) and write profiles/transformer.txt.

Three attention paths inside the SAME modules (dense layers on the split-fp16 GEMM, fused norm + residual, everything else alike):

    fused      ops.attention.attention (csrc/attention.hip)
    composed   torch.matmul + log-mask + softmax + matmul, the reference's formulation (transformer.py:28-38): materialises [B, H, T, T]
    library    F.scaled_dot_product_attention with a boolean key mask

Per size: forward (no_grad) and forward + backward, eager and replayed from a graph; the median of ``--reps`` timed runs after
``--warmup`` (HIP events around each run, one synchronisation per run).  No number here is gated.

    python scripts/bench_transformer.py [--sizes 250,1000] [--reps 10] [--warmup 3] [--out profiles/transformer.txt]
"""
import argparse
import math
import statistics
import sys
from pathlib import Path

REPO = Path(__file__).resolve().parent.parent
if str(REPO) not in sys.path:
    sys.path.insert(0, str(REPO))

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402


def composed(q, k, v, lengths=None, causal=False, mask=None, need_weights=False):
    y = q @ k.transpose(-2, -1) / math.sqrt(k.shape[-1])
    if lengths is not None:
        keep = torch.arange(k.shape[2], device=q.device)[None, None, None, :] < lengths[:, None, None, None]
        y = y + torch.log(keep.float())
    if causal:
        y = y + torch.log(torch.tril(torch.ones_like(y), diagonal=y.shape[-1] - y.shape[-2]))
    y = torch.softmax(y, dim=-1)
    return y @ v, None


def library(q, k, v, lengths=None, causal=False, mask=None, need_weights=False):
    keep = None
    if lengths is not None:
        keep = torch.arange(k.shape[2], device=q.device)[None, None, None, :] < lengths[:, None, None, None]
    return F.scaled_dot_product_attention(q, k, v, attn_mask=keep, is_causal=causal), None


def timed(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1))
    return statistics.median(times), min(times), max(times)


def captured(fn):
    from padertorch_amd.ops import capture
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        fn()
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with capture.capture_mode():
        with torch.cuda.graph(graph, stream=side):
            capture.zero_block(torch.device('cuda', torch.cuda.current_device()))
            fn()
    return graph.replay


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--sizes', default='250,1000')
    ap.add_argument('--reps', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--out', default=str(REPO / 'profiles' / 'transformer.txt'))
    args = ap.parse_args()
    from padertorch_amd import _lib
    from padertorch_amd.contrib.je.modules import TransformerLayerStack
    from padertorch_amd.contrib.je.modules import transformer as tf
    from padertorch_amd.ops import attention as att

    dev = torch.device('cuda:0')
    B, d_in, d, d_ff, H, L = 16, 80, 512, 2048, 8, 6
    torch.manual_seed(0)
    net = TransformerLayerStack(d_in, d, d_ff, H, L, bidirectional=True).to(dev)
    params = list(net.parameters())
    fused = att.attention
    paths = (('fused', fused), ('composed', composed), ('library', library))
    lib = _lib.load()
    lines = [f'# transformer stack: input {d_in}, hidden_size {d}, {H} heads of {d // H}, d_ff {d_ff}, {L} layers, B = {B}, bidirectional, '
             f'lengths T/2 .. T; {torch.cuda.get_device_name(0)}; median (min .. max) ms of {args.reps} runs after {args.warmup}',
             f'# attention tile: a workgroup owns {lib.ptmi_attn_tile()} rows (16 per wave) and streams tiles of {lib.ptmi_attn_key_tile()} rows; '
             'the only tile compiled - no sweep over tile sizes was run',
             f'{"T":>5s} {"path":9s} {"pass":18s} {"eager ms":>28s} {"replayed ms":>28s}']
    for T in (int(s) for s in args.sizes.split(',')):
        x = torch.randn(B, T, d_in, device=dev)
        w = torch.randn(B, T, d, device=dev)
        lengths = torch.linspace(T // 2, T, B).round().to(torch.int32).to(dev)
        results = {}
        for name, fn in paths:
            class Patched:
                attention = staticmethod(fn)

                def __getattr__(self, item):
                    return getattr(att, item)
            tf._attn = att if fn is fused else Patched()

            def forward():
                with torch.no_grad():
                    return net(x, lengths)[0]
            xg = x.clone().requires_grad_()

            def both():
                y, _ = net(xg, lengths)
                return torch.autograd.grad((y * w).sum(), [xg] + params)
            for label, step in (('forward', forward), ('forward + backward', both)):
                eager = timed(step, args.reps, args.warmup)
                replay = timed(captured(step), args.reps, args.warmup)
                results[name, label] = (eager, replay)
                lines.append(f'{T:5d} {name:9s} {label:18s} ' + ' '.join(f'{m:9.3f} ({lo:7.3f} .. {hi:7.3f})' for m, lo, hi in (eager, replay)))
                print(lines[-1], flush=True)
            tf._attn = att
        for label in ('forward', 'forward + backward'):
            f_ = results['fused', label]
            lines.append(f'{T:5d} {"":9s} {label:18s} fused / composed: eager {f_[0][0] / results["composed", label][0][0]:.2f}, replayed '
                         f'{f_[1][0] / results["composed", label][1][0]:.2f};  fused / library: eager '
                         f'{f_[0][0] / results["library", label][0][0]:.2f}, replayed {f_[1][0] / results["library", label][1][0]:.2f}')
            print(lines[-1], flush=True)
    out = Path(args.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text('\n'.join(lines) + '\n')
    print(out)


if __name__ == '__main__':
    main()
