#!/usr/bin/env python3
"""Time the Conv-TasNet separator: forward + backward of one gLN block (dilation 1 and 128), of the block's non-GEMM region
(PReLU -> pad -> depthwise conv -> PReLU -> gLN) and of the whole default ``ConvNet()`` (256 / 512 / K = 3 / 8 x 4) at B = 4, T = 3199
(4 s at 8 kHz behind the convnet coder row of profiles/tas_coders.txt), on the HIP kernels (padertorch_amd.ops.tcn + the split-fp16
GEMM) and on the torch library path - the same parameters composed from F.conv1d (1x1 and ``groups``), F.prelu and torch.mean on
``[B, C, T]`` - on the same GPU in the same process.  The depthwise forward launch is also timed alone and reported as bytes / s
against its algorithmic traffic (8 bytes per element) and against the ~5 TB/s a copy reaches on this part.

    python scripts/bench_convnet.py [--iters 20] [--warmup 5] [--rounds 5] [--out profiles/convnet.txt]

Method (as scripts/bench_tas_coders.py): every chain is warmed up, then timed in ``rounds`` windows of ``iters`` iterations between two
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

B, T = 4, 3199


def gln(x, norm):            # x [B, C, T]
    mean = torch.mean(x, (1, 2), keepdim=True)
    var = torch.mean((x - mean) ** 2, (1, 2), keepdim=True)
    return norm.gamma * (x - mean) / torch.sqrt(var + norm.eps) + norm.beta


def library_region(block, u):            # u [B, H, T]
    from padertorch_amd.ops.tcn import depthwise_pad
    c = block.conv
    p = F.pad(F.prelu(u, block.input_conv.activation_fn.weight), depthwise_pad(c.kernel_size, c.dilation))
    v = F.prelu(F.conv1d(p, c.conv.weight, c.conv.bias, dilation=c.dilation, groups=u.shape[1]), c.activation_fn.weight)
    return gln(v, block.norm)


def library_block(block, x):             # x [B, C, T]
    u = F.conv1d(gln(x, block.input_norm), block.input_conv.conv.weight, block.input_conv.conv.bias)
    return x + F.conv1d(library_region(block, u), block.output_conv.conv.weight, block.output_conv.conv.bias)


def hip_region(block, u):                # u [B, T, H]
    from padertorch_amd.ops import tcn
    c = block.conv
    v, stats = tcn.depthwise_prelu(u, block.input_conv.activation_fn.weight, c.conv.weight, c.conv.bias, c.activation_fn.weight,
                                   c.dilation, c.kernel_size)
    return block.norm(v, stats)


def chain(fn, x, params):
    r = torch.randn_like(fn(x).detach())

    def run():
        return torch.autograd.grad((fn(x) * r).sum(), [x] + params)
    return run


def window(fn, iters):
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(iters):
        fn()
    end.record()
    end.synchronize()
    return start.elapsed_time(end) * 1e3 / iters        # us per iteration


def measure(name, series, args, extra=None):
    for fn in series.values():
        for _ in range(args.warmup):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in series}
    for _ in range(args.rounds):
        for k, fn in series.items():
            times[k].append(window(fn, args.iters))
    res = dict(what=name, **{k: dict(median_us=round(statistics.median(t), 1), min_us=round(min(t), 1), max_us=round(max(t), 1))
                             for k, t in times.items()})
    if 'library' in res:
        res['hip_no_slower'] = res['hip']['median_us'] <= res['library']['median_us']
    res.update(extra(res) if extra else {})
    print(json.dumps(res), flush=True)
    return json.dumps(res)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_convnet.py needs an MI355X'
    from padertorch_amd.modules import ConvNet
    from padertorch_amd.modules.convnet import _Conv1DBlock
    dev = torch.device('cuda:0')
    torch.manual_seed(0)
    lines = []
    for d in (1, 128):
        block = _Conv1DBlock(256, 512, 3, dilation=d, norm='gLN').to(dev)
        params = list(block.parameters())
        x = torch.randn(B, T, 256, device=dev, requires_grad=True)
        xt = x.detach().transpose(1, 2).contiguous().requires_grad_()
        hip, lib = chain(block, x, params), chain(lambda t: library_block(block, t), xt, params)
        worst = max(float((a - b).abs().max() / b.abs().max()) for a, b in zip(hip()[1:], lib()[1:]))
        print(f'd={d}: parameter gradients of the two chains differ by at most {worst:.1e} of their maximum', flush=True)
        assert worst <= 1e-2, (d, worst)                     # the two chains compute the same thing (both fp32)
        lines.append(measure(f'gLN block 256/512/3 d={d} B={B} T={T}, forward + backward', dict(hip=hip, library=lib), args))
        u = torch.randn(B, T, 512, device=dev, requires_grad=True)
        ut = u.detach().transpose(1, 2).contiguous().requires_grad_()
        region = [block.input_conv.activation_fn.weight, block.conv.conv.weight, block.conv.conv.bias, block.conv.activation_fn.weight,
                  block.norm.gamma, block.norm.beta]
        lines.append(measure(f'non-GEMM region (prelu, pad, depthwise, prelu, gLN) 512 d={d} B={B} T={T}, forward + backward',
                             dict(hip=chain(lambda t: hip_region(block, t), u, region),
                                  library=chain(lambda t: library_region(block, t), ut, region)), args))
        c, ud = block.conv, u.detach()

        @torch.no_grad()
        def fwd():
            return torch.ops.ptmi.tcn_depthwise_forward(ud, block.input_conv.activation_fn.weight, c.conv.weight, c.conv.bias,
                                                        c.activation_fn.weight, d, 1e-5)

        def rate(res):
            tbs = 8. * ud.numel() / (res['hip']['median_us'] * 1e-6) / 1e12
            return dict(algorithmic_bytes=8 * ud.numel(), achieved_TBps=round(tbs, 3), of_a_5TBps_copy=round(tbs / 5., 3))
        lines.append(measure(f'depthwise forward launch (+ statistics finalize) 512 d={d} B={B} T={T}', dict(hip=fwd), args, rate))
    net = ConvNet().to(dev)
    params = list(net.parameters())
    x = torch.randn(B, T, 256, device=dev, requires_grad=True)
    xt = x.detach().transpose(1, 2).contiguous().requires_grad_()

    def library_net(t):
        for rep in net.conv_blocks:
            for block in rep:
                t = library_block(block, t)
        return t
    lines.append(measure(f'ConvNet() default (256/512/3/8x4 gLN) B={B} T={T}, forward + backward',
                         dict(hip=chain(net, x, params), library=chain(library_net, xt, params)), args))
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
