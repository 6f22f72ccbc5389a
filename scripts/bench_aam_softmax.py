"""The fused angular-margin softmax head (``ops.aam_softmax``, ``csrc/aam_softmax.hip``) against two torch formulations, forward and
forward + backward, eager and graph replay, at ``B = 256, E = 256`` with ``C = 5994`` (VoxCeleb2) and ``C = 100 000``.

    (a) vectorised torch: F.normalize, F.linear, a masked logsumexp          (library GEMM, [B, C] logits through HBM)
    (b) the reference's literal formulation (loss.py:79-103): diagonal gather and its Python loop of B torch.cat (not capturable:
        the loop slices with host integers)

Times are device events around ``--iters`` calls after a warm-up, the median of ``--repeats`` windows; the share of HBM bandwidth is the
bytes the algorithm needs (W read and written once by the normalisation, read once by the GEMM; in the backward read twice, dW written
once) over the time, against the 8.0 TB/s of the MI355X's data sheet.  ``python scripts/bench_aam_softmax.py > profiles/aam_softmax.txt``
"""
import argparse
import statistics
import sys
from pathlib import Path

import torch
import torch.nn.functional as F

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from padertorch_amd.ops.aam_softmax import angular_softmax_loss  # noqa: E402

PEAK = 8.0e12
S, M = 30.0, 0.2


def ours(e, w, y):
    return angular_softmax_loss(e, w, y, 'aam', check=False)


def vectorised(e, w, y):
    w.data = F.normalize(w, p=2, dim=1)
    logits = S * F.linear(F.normalize(e, p=2, dim=1), w)
    n = logits.gather(1, y[:, None])[:, 0] - S * M
    others = logits.scatter(1, y[:, None], float('-inf'))
    return -(n - torch.logsumexp(torch.cat([n[:, None], others], 1), 1)).mean()


def literal(e, w, y):
    w.data = F.normalize(w, p=2, dim=1)
    logits = F.linear(F.normalize(e, p=2, dim=1), w)
    numerator = S * (torch.diagonal(logits.transpose(1, 0)[y]) - M)
    excl = torch.cat([torch.cat((logits[i, :t], logits[i, t + 1:])).unsqueeze(0) for i, t in enumerate(y)], dim=0)
    L = numerator - torch.log(torch.exp(numerator) + torch.sum(torch.exp(S * excl), dim=1))
    return -torch.mean(L)


def window(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / iters


def measure(fn, iters, repeats):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    return statistics.median(window(fn, iters) for _ in range(repeats))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=50)
    ap.add_argument('--repeats', type=int, default=5)
    ap.add_argument('--classes', type=int, nargs='+', default=[5994, 100000])
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'needs an MI355X: no CPU timing says anything about it'
    B = E = 256
    print(f'# {torch.cuda.get_device_name(0)}; B = {B}, E = {E}, aam s = {S} m = {M}; us per call, median of {args.repeats} windows of '
          f'{args.iters} calls\n# {"C":>7} {"path":<12}{"fwd eager":>11}{"fwd graph":>11}{"f+b eager":>11}{"f+b graph":>11}   HBM share of f+b graph')
    for C in args.classes:
        g = torch.Generator().manual_seed(C)
        e = torch.randn(B, E, generator=g).cuda().requires_grad_(True)
        w0 = F.normalize(torch.randn(C, E, generator=g), dim=1).cuda()
        y = torch.randint(0, C, (B,), generator=g).cuda()
        need = 4 * C * E * (3 + 3)                          # forward: W read, written, read; backward: W read twice, dW written
        for name, fn in (('hip fused', ours), ('torch vector', vectorised), ('torch literal', literal)):
            w = w0.clone().requires_grad_(True)
            iters = args.iters if name != 'torch literal' else max(args.iters // 10, 2)

            def fwd():
                with torch.no_grad():
                    return fn(e, w, y)

            def both():
                return torch.autograd.grad(fn(e, w, y), (e, w))
            row = [measure(fwd, iters, args.repeats), None, measure(both, iters, args.repeats), None]
            if name != 'torch literal':
                for k, step in ((1, fwd), (3, both)):
                    graph = torch.cuda.CUDAGraph()
                    side = torch.cuda.Stream()
                    side.wait_stream(torch.cuda.current_stream())
                    with torch.cuda.stream(side):
                        step()
                    torch.cuda.current_stream().wait_stream(side)
                    with torch.cuda.graph(graph):
                        step()
                    row[k] = measure(graph.replay, iters, args.repeats)
            cells = ''.join(f'{v:>11.1f}' if v is not None else f'{"-":>11}' for v in row)
            share = f'{need / (row[3] * 1e-6) / PEAK:7.1%} of 8.0 TB/s ({need / 1e6:.0f} MB needed)' if row[3] else 'not capturable'
            print(f'{C:>9} {name:<12}{cells}   {share}')


if __name__ == '__main__':
    main()
