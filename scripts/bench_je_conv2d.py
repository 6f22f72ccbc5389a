#!/usr/bin/env python3
"""Time contrib/je's 2-D convolution stack: forward and forward + backward, eagerly and as a replayed ``torch.cuda.graph``, at ``B = 16``,
``T = 512`` for

    single blocks at WALNet's plane sizes: Conv2d(C_in, C_out, 3, norm='batch') (relu, pad 'both') for
        1 -> 16 at F = 128,  16 -> 16 at F = 128,  64 -> 64 at F = 32,  256 -> 256 at F = 8
    WALNet's whole CNN2d (13 layers, 1 -> 16 -> ... -> 1024 -> output_size 10, 2 x 2 max pools, 128 mel bins)

Every row is compared with the library composition on the same GPU in the same process, built from the SAME parameters: ``F.pad``,
``F.conv2d`` (MIOpen), this package's ``Normalization``, the torch activation, ``F.max_pool2d``.  No lengths (a graph needs none).

    python scripts/bench_je_conv2d.py [--iters 10] [--warmup 3] [--rounds 5] [--out profiles/je_conv2d.txt]

Method: scripts/bench_je_conv.py's (``timed``, ``chain``, ``graphed`` are that script's).  Rows where the library is faster are printed in
bold (``**...**``).  Needs a GPU.
"""
import argparse
import sys
from pathlib import Path

import torch
import torch.nn.functional as F

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
sys.path.insert(0, str(Path(__file__).resolve().parent))

from bench_je_conv import chain, graphed, timed  # noqa: E402

B, T = 16, 512
BLOCKS = {'1 -> 16, F 128': (1, 16, 128), '16 -> 16, F 128': (16, 16, 128), '64 -> 64, F 32': (64, 64, 32), '256 -> 256, F 8': (256, 256, 8)}
WALNET = dict(in_channels=1, out_channels=[16, 16, 32, 32, 64, 64, 128, 128, 256, 256, 512, 1024, 10], kernel_size=11 * [3] + [2, 1],
              pad_type=11 * ['both'] + 2 * [None], pool_size=[1, 2, 1, 2, 1, 2, 1, 2, 1, 2, 2, 1, 1], norm='batch', activation_fn='relu')


def library_block(m, x):
    """One ``Conv2d`` block of the reference's formulation on library kernels, with the module's own parameters."""
    from padertorch_amd.contrib.je.modules.conv_utils import compute_pad_size
    (ff, fe), (tf, te) = (compute_pad_size(k, d, s, p) for k, d, s, p in zip(m.kernel_size, m.dilation, m.stride, m.pad_type))
    y = F.conv2d(F.pad(x, (tf, te, ff, fe)), m.conv.weight, m.conv.bias, stride=m.stride, dilation=m.dilation)
    if m.norm is not None:
        y = m.norm(y)
    return m.activation_fn(y)


def library_cnn(net, x):
    from padertorch_amd.contrib.je.modules.conv_utils import compute_pad_size, to_pair
    for i, conv in enumerate(net.convs):
        x = library_block(conv, x)
        size = to_pair(net.pool_sizes[i])
        if max(size) > 1:
            (ff, fe), (tf, te) = (compute_pad_size(k, 1, k, p) for k, p in zip(size, to_pair(net.pad_types[i])))
            x = F.max_pool2d(F.pad(x, (tf, te, ff, fe)), size)
    return x


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    from padertorch_amd.contrib.je.modules import CNN2d, Conv2d
    lines = [f'contrib/je Conv2d / CNN2d, B = {B}, T = {T}, norm = batch, relu, fp32; us per iteration: median (min .. max) of {args.rounds} '
             f'windows of {args.iters}; ratio = library / ours (above 1: ours is faster; bold: the library is faster)',
             torch.cuda.get_device_name(0), '']
    subjects = {}
    for name, (c_in, c_out, f) in BLOCKS.items():
        torch.manual_seed(0)
        m = Conv2d(c_in, c_out, 3, norm='batch').cuda()
        subjects[name] = (lambda v, m=m: m(v)[0], lambda v, m=m: library_block(m, v), list(m.parameters()), (B, c_in, f, T))
    torch.manual_seed(0)
    net = CNN2d(**WALNET).cuda()
    subjects['WALNet CNN2d'] = (lambda v: net(v)[0], lambda v: library_cnn(net, v), list(net.parameters()), (B, 1, 128, T))
    for name, (ours, lib, ps, shape) in subjects.items():
        x = torch.randn(*shape, device='cuda', requires_grad=True)
        for backward in (False, True):
            eager = {'ours': chain(ours, x, ps, backward), 'library': chain(lib, x, ps, backward)}
            chains = dict(eager)
            for k, fn in eager.items():
                chains[k + ' graph'] = graphed(fn)
            res = timed(chains, args.iters, args.warmup, args.rounds)
            for mode in ('', ' graph'):
                a, b = res['ours' + mode], res['library' + mode]
                row = (f'{name:16s} {"fwd+bwd" if backward else "fwd    "} {"graph" if mode else "eager"}  '
                       f'ours {a[0]:9.1f} ({a[1]:9.1f} .. {a[2]:9.1f})   library {b[0]:9.1f} ({b[1]:9.1f} .. {b[2]:9.1f})   '
                       f'ratio {b[0] / a[0]:5.2f}')
                lines.append(f'**{row}**' if b[0] < a[0] else row)
                print(lines[-1], flush=True)
    text = '\n'.join(lines) + '\n'
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(text)
    else:
        print(text)


if __name__ == '__main__':
    main()
