#!/usr/bin/env python3
"""Time the fixed-basis STFT coders (``ops/stft_coders.py``) at the size of the reference's ``stft`` TasNet configuration - B 4, T 32000,
L 16, N 64 (hop 8, 3999 frames), K 2 - against the same computation composed from what the project offered before them: ``ops.STFT``
(``[B, frames, bins]``, so the coder transposes), ``mask * encoded`` in torch, ``STFT.inverse``.  Encode, masked decode and their
backwards (gradients in the signal, the masks and the encoded signal).  Next to them the whole ``stft`` + ConvNet and ``stft`` + DPRNN
steps (forward + backward of ``sum(out r)``) and their learned-coder twins (``TasEncoder`` / ``TasDecoder``, which also compute the
basis gradients).

    python scripts/bench_stft_tasnet.py [--iters 10] [--warmup 3] [--rounds 5] [--out profiles/stft_tasnet.txt]

Method (as scripts/bench_convnet.py): every chain is warmed up, then timed in ``rounds`` windows of ``iters`` iterations
between two events, the chains alternating window by window; reported are the median window (us per iteration) and min .. max.  Needs
a GPU.
"""
import argparse
import json
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

from scripts.bench_dprnn import timed  # noqa: E402

B, T, L, N, K = 4, 32000, 16, 64, 2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    from padertorch_amd.contrib.examples.source_separation.tasnet import IstftDecoder, StftEncoder, TasDecoder, TasEncoder, TasNet
    from padertorch_amd.modules import DPRNN, ConvNet
    torch.manual_seed(0)
    enc, dec = StftEncoder(L, N).cuda(), IstftDecoder(L, N).cuda()
    x = torch.randn(B, T, device='cuda', requires_grad=True)
    E = enc(x).shape[-1]
    mask = torch.rand(K, B, N, E, device='cuda', requires_grad=True)
    g = torch.randn(K, B, (E - 1) * (L // 2) + L, device='cuda')

    def fixed():
        e = enc(x)
        return torch.autograd.grad((dec.masked(mask, e) * g).sum(), [x, mask])

    def composed():
        e = enc.stft(x).transpose(-1, -2)                                  # [B, N, E], a view
        y = dec.stft.inverse((mask * e).reshape(K * B, N, E).transpose(-1, -2)).view(K, B, -1)
        return torch.autograd.grad((y * g).sum(), [x, mask])

    a, b = fixed(), composed()
    agree = [float((p - q).abs().max() / q.abs().max()) for p, q in zip(a, b)]
    chains = {'coders fwd+bwd, fixed basis (stft_encode, istft_masked_decode)': fixed,
              'coders fwd+bwd, composed (ops.STFT, mask * encoded, STFT.inverse)': composed}
    r = torch.randn(B, K, T, device='cuda')
    lengths = torch.tensor([T, T - 100, T - 150, T // 2], device='cuda')

    def step_of(net):
        net = net.cuda()
        leaves = list(net.parameters())

        def run():
            return torch.autograd.grad((net(dict(y=x, num_samples=lengths))['out'] * r).sum(), leaves)
        return run

    for name, sep in (('convnet', lambda: ConvNet(input_size=N)), ('dprnn', lambda: DPRNN(N, 128, 100, 50, 6))):
        chains[f'step fwd+bwd, stft + {name}'] = step_of(TasNet(StftEncoder(L, N), sep(), IstftDecoder(L, N)))
        chains[f'step fwd+bwd, learned coders + {name}'] = step_of(TasNet(TasEncoder(L, N), sep(), TasDecoder(L, N)))
    res = timed(chains, args.iters, args.warmup, args.rounds)
    lines = [f'STFT-domain TasNet coders: B {B}, T {T}, L {L}, N {N}, hop {L // 2}, {E} frames, K {K}; {torch.cuda.get_device_name(0)}',
             f'method: {args.warmup} warm-up iterations, then {args.rounds} windows of {args.iters} iterations per chain between two events, '
             'the chains alternating; us per iteration, median window (min .. max)',
             'fixed against composed, max |difference| / max |composed|: d x %.2e, d mask %.2e' % tuple(agree), '']
    for k, v in res.items():
        lines.append(f'{k:72s} {v["median_us"]:10.1f}  ({v["min_us"]:.1f} .. {v["max_us"]:.1f})')
    f, c = (res[k]['median_us'] for k in list(chains)[:2])
    lines += ['', f'coders: fixed basis / composed = {f / c:.3f} ' + ('(the fixed-basis path is the faster one)' if f < c else
              '(the fixed-basis path is NOT the faster one here; it is kept for what it avoids: the product mask * encoded in memory and '
              'the two transposed copies, and for a step that captures in a graph)'), json.dumps(res)]
    text = '\n'.join(lines) + '\n'
    print(text)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(text)


if __name__ == '__main__':
    main()
