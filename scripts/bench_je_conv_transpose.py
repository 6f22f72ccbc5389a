#!/usr/bin/env python3
"""Time contrib/je's transposed convolution stack: forward and forward + backward, eagerly and as a replayed ``torch.cuda.graph``, at
``B = 16`` for

    single blocks ConvTranspose2d(C, C, k, stride=(2, 2), norm='batch') (relu, pad 'both'), k = 3 and 4:
        narrow  16 -> 16,   F 64 -> 128, T 256 -> 512
        wide    256 -> 256, F 4 -> 8,    T 256 -> 512
    ConvTranspose1d(256, 256, k, stride=2, norm='batch'), T 256 -> 512
    the CNNTranspose2d that get_transpose_config mirrors from WALNet's CNN2d (scripts/bench_je_conv2d.py), from that network's output plane

against two baselines on the same GPU in the same process, built from the SAME parameters:

    library         F.conv_transpose2d / F.conv_transpose1d (MIOpen), this package's Normalization on the untrimmed output, the torch
                    activation, the trim as a slice; F.interpolate where the stack unpools
    zero insertion  the same block through the route the package had before the phase kernel: torch.ops.ptmi.je_conv2d_forward with
                    input-gradient planes (the input is staged with zeros between its values and every tap runs over them), then the
                    same statistics / apply launches.  Forward only: its backward would be the very launches of ours.

Beside the times: matrix-instruction k steps (32 wide) per output pixel and 16 output channels, by arithmetic - the phase kernel's sum
over the phases divided by the pixels of a phase cell, and zero insertion's ``chunks ceil(K_f K_t (CC / 8) / 4)``.

    python scripts/bench_je_conv_transpose.py [--iters 10] [--warmup 3] [--rounds 5] [--out profiles/je_conv_transpose.txt]

Method: scripts/bench_je_conv.py's (``timed``, ``chain``, ``graphed`` are that script's): medians of windows.  Rows where the library is
faster are printed in bold (``**...**``).  No lengths (a graph needs none).  Needs a GPU.
"""
import argparse
import sys
from pathlib import Path

import torch
import torch.nn.functional as F

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
sys.path.insert(0, str(Path(__file__).resolve().parent))

from bench_je_conv import chain, graphed, timed  # noqa: E402
from bench_je_conv2d import WALNET  # noqa: E402

B = 16
#: name -> (channels, input plane); a plane of one number: the 1-D class
BLOCKS = {'narrow 16 -> 16, F 64 -> 128': (16, (64, 256)), 'wide 256 -> 256, F 4 -> 8': (256, (4, 256)), '1-D 256 -> 256': (256, (256,))}


def geometry(m, plane):
    """Per axis ``(kernel, stride, dilation, front, full, trimmed)`` of a block on an input plane ``(F, T)``."""
    from padertorch_amd.contrib.je.modules.conv_utils import compute_pad_size
    out = []
    for n, k, s, d, p in zip(plane, *m._axes()):
        front, end = compute_pad_size(k, d, s, p)
        full = (n - 1) * s + d * (k - 1) + 1
        out.append((k, s, d, front, full, full - front - max(end - s + 1, 0)))
    return out


def library_block(m, x):
    """One transposed block of the reference's formulation on library kernels, with the module's own parameters."""
    four = x if m.is_2d() else x.unsqueeze(2)
    kernel, stride, dilation, _ = m._axes()
    w = m.conv.weight if m.is_2d() else m.conv.weight.unsqueeze(2)
    y = F.conv_transpose2d(four, w, m.conv.bias, stride=stride, dilation=dilation)
    y = y if m.is_2d() else y.squeeze(2)
    if m.norm is not None:
        y = m.norm(y)
    y = m.activation_fn(y)
    geo = geometry(m, tuple(four.shape[2:]))
    index = [slice(None), slice(None)] + [slice(g[3], g[3] + g[5]) for g in (geo if m.is_2d() else geo[1:])]
    return y[tuple(index)]


def zero_insertion_block(m, x):
    """The block's forward through ``je_conv2d_forward`` in its input-gradient mode (zeros inserted in LDS), no gradient."""
    from padertorch_amd.contrib.je.modules.conv import _norm_operands
    from padertorch_amd.contrib.je.modules.conv_utils import activation_code
    from padertorch_amd.ops import je_conv2d as ops2
    ops = torch.ops.ptmi
    with torch.no_grad():
        rows, B_, F_in, T_in = ops2.planes(x if m.is_2d() else x.unsqueeze(2))
        (kf, sf, df, _, full_f, _), (kt, st, dt, _, full_t, _) = geo = geometry(m, (F_in, T_in))
        if not hasattr(m, 'w4'):        # one tensor object per module: je_conv2d's plane cache is keyed on it
            m.w4 = m.conv.weight.detach() if m.is_2d() else m.conv.weight.detach().unsqueeze(2)
        w = m.w4
        geom = [B_, F_in, T_in, m.in_channels, 1, sf, st, full_f, full_t, m.out_channels, 1, kf, kt, 1, 1, df, dt, (kf - 1) * df, (kt - 1) * dt]
        planes, amax_w = ops2._planes_form(w, None, geom, True)
        z = ops.je_conv2d_forward(rows, None, planes, ops2._word(rows), amax_w, m.conv.bias, None, None, None, geom, 0, 0., False)[0]
        code, p, slope = activation_code(m.activation_fn)
        kind, fixed = _norm_operands(m.norm)
        stats = fixed if fixed is not None else ops.je_conv_stats(z, None, B_ * full_f, full_t, kind == 'sequence', m.norm.eps)
        y = ops.je_conv_apply(z, None, None, stats, m.norm.gamma.reshape(-1), m.norm.beta.reshape(-1), None, slope, B_ * full_f, full_t,
                              kind == 'sequence', code, p)
        y = ops2.unplanes(y, B_, full_f, full_t)[:, :, geo[0][3]:geo[0][3] + geo[0][5], geo[1][3]:geo[1][3] + geo[1][5]]
        return y if m.is_2d() else y.squeeze(2)


def library_cnn(net, x):
    from padertorch_amd.contrib.je.modules.conv_utils import to_pair
    for i, conv in enumerate(net.convs):
        if max(to_pair(net.pool_sizes[i])) > 1:
            x = F.interpolate(x, scale_factor=to_pair(net.pool_strides[i]))
        x = library_block(conv, x)
    return x


def k_steps(m, plane):
    """``(phase kernel, zero insertion)``: k steps per output pixel and 16 output channels, all channel chunks."""
    from padertorch_amd.ops import je_conv_transpose as opst
    (kf, sf, df, _, full_f, _), (kt, st, dt, _, full_t, _) = geometry(m, plane)
    cfg = opst.TransposeConfig(B, *plane, full_f, full_t, (kf, kt), (sf, st), (df, dt), (0, 0), None, 0., 0, 0., False)
    cp = -(-m.in_channels // 8) * 8
    cc = 32 if cp >= 32 else (16 if cp >= 16 else 8)
    return opst.ksteps(opst.plan(cfg, m.in_channels, m.out_channels, 1)) / (sf * st), -(-cp // cc) * -(-kf * kt * (cc // 8) // 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    from padertorch_amd.contrib.je.modules import CNN2d
    from padertorch_amd.contrib.je.modules import conv_transpose as ct
    lines = [f'contrib/je ConvTranspose / CNNTranspose2d, B = {B}, stride 2, norm = batch, relu, fp32; us per iteration: median (min .. max) '
             f'of {args.rounds} windows of {args.iters}; ratio = baseline / ours (above 1: ours is faster; bold: the library is faster); '
             f'k steps per output pixel and 16 output channels by arithmetic', torch.cuda.get_device_name(0), '']
    subjects = {}
    for name, (c, plane) in BLOCKS.items():
        for k in (3, 4):
            torch.manual_seed(0)
            two = len(plane) == 2
            m = (ct.ConvTranspose2d if two else ct.ConvTranspose1d)(c, c, k, stride=2, norm='batch').cuda()
            ks = k_steps(m, plane if two else (1, *plane))
            subjects[f'{name}, k {k}'] = (lambda v, m=m: m(v)[0], lambda v, m=m: library_block(m, v), lambda v, m=m: zero_insertion_block(m, v),
                                          list(m.parameters()), (B, c, *plane), f'k steps {ks[0]:.2f} against {ks[1]}')
    torch.manual_seed(0)
    mirror = ct.get_transpose_config(dict(WALNET, factory=CNN2d))
    net = mirror.pop('factory')(**mirror).cuda()
    start = tuple(int(n) for n in CNN2d(**WALNET).get_shapes(input_shape=(B, 1, 128, 512))[-1])
    subjects['mirrored WALNet CNNTranspose2d'] = (lambda v: net(v)[0], lambda v: library_cnn(net, v), None, list(net.parameters()), start,
                                                  f'from {start[2]} x {start[3]}')
    for name, (ours, lib, zero, ps, shape, note) in subjects.items():
        x = torch.randn(*shape, device='cuda', requires_grad=True)
        try:
            ours(x)
        except NotImplementedError as e:            # a geometry a planner refuses is a row, not the end of the table
            lines.append(f'{name}: refused: {e}')
            print(lines[-1], flush=True)
            continue
        with torch.no_grad():           # the three routes compute the same thing
            want = ours(x)
            note += ''.join(f', max |ours - {k}| {float((fn(x) - want).abs().max()):.1e}' for k, fn in (('library', lib), ('zero insertion', zero))
                            if fn is not None) + f' at max |ours| {float(want.abs().max()):.1f}'
        lines.append(f'{name}: {note}')
        print(lines[-1], flush=True)
        for backward in (False, True):
            eager = {'ours': chain(ours, x, ps, backward), 'library': chain(lib, x, ps, backward)}
            if zero is not None and not backward:
                eager['zero insertion'] = lambda zero=zero, x=x: zero(x)
            chains = dict(eager)
            for k, fn in eager.items():
                chains[k + ' graph'] = graphed(fn)
            res = timed(chains, args.iters, args.warmup, args.rounds)
            for mode in ('', ' graph'):
                a, b = res['ours' + mode], res['library' + mode]
                row = (f'  {"fwd+bwd" if backward else "fwd    "} {"graph" if mode else "eager"}  ours {a[0]:9.1f} ({a[1]:9.1f} .. {a[2]:9.1f})   '
                       f'library {b[0]:9.1f} ({b[1]:9.1f} .. {b[2]:9.1f})   ratio {b[0] / a[0]:5.2f}')
                if 'zero insertion' + mode in res:
                    z = res['zero insertion' + mode]
                    row += f'   zero insertion {z[0]:9.1f} ({z[1]:9.1f} .. {z[2]:9.1f})   ratio {z[0] / a[0]:5.2f}'
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
