#!/usr/bin/env python3
"""Time the mask estimator's loss (``ops.mask_bce_loss``: csrc/mask_loss.hip), forward + backward, at ``B 8, C 6, T 600, F 513`` with
ragged lengths, for ``mean`` and ``median``, with and without the observation's power, against the torch composition of the
reference's formula (``contrib/jensheit/mask_estimator_example/model.py:128-237``: per example
``F.binary_cross_entropy_with_logits(reduction='none')``, ``torch.mean`` / ``torch.median``, ``sum(l w) / sum(w)``, autograd) on the
same tensors and GPU in the same process.  The composition gets the power weights ``|stft|^2`` made on the device (the reference makes
them on the host with numpy and copies them over at every review: that copy is NOT in its time here).

    python scripts/bench_mask_loss.py [--iters 20] [--warmup 5] [--rounds 5] [--out profiles/mask_loss.txt]

Method (scripts/bench_convnet.py): every chain is warmed up, then timed in ``rounds`` windows of ``iters`` iterations between two events,
the chains alternating window by window; reported are the median window (us per iteration) and min .. max.  ``algorithmic_bytes``: what
one forward and one backward pass over the data need - logits and target (and the complex power) of the valid frames read twice, the
dense gradient written once; ``achieved_GBs`` is that over the fused op's time (a whole-call rate, launches and the selection's extra
passes included - not a kernel's share of peak).  The outputs of the two chains are compared at the timed size first.  Needs a GPU.
"""
import argparse
import sys
from pathlib import Path

import torch
import torch.nn.functional as F

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
sys.path.insert(0, str(Path(__file__).resolve().parent))

from bench_convnet import measure  # noqa: E402

B, C, T, NF = 8, 6, 600, 513
FRAMES = [600, 571, 533, 502, 467, 431, 388, 342]
HBM_GBS = 8000.     # MI355X peak HBM bandwidth, GB/s
POOL = dict(mean=torch.mean, median=torch.median)


def library_step(logits, target, power, reduction, gp, gw):
    """The reference's loop: ``(pooled [B], weighted [B] or None, d logits)``."""
    x = logits.detach().requires_grad_()
    pooled, weighted = [], []
    for b, n in enumerate(FRAMES):
        loss = F.binary_cross_entropy_with_logits(x[b, :, :n], target[b, :, :n], reduction='none')
        pooled.append(POOL[reduction](loss))
        if power is not None:
            w = power[b, :, :n].abs() ** 2
            weighted.append(torch.sum(loss * w) / torch.sum(w))
    pooled = torch.stack(pooled)
    total = (pooled * gp).sum()
    if power is not None:
        weighted = torch.stack(weighted)
        total = total + (weighted * gw).sum()
    grad, = torch.autograd.grad(total, x)
    return pooled.detach(), (weighted.detach() if power is not None else None), grad


def hip_step(logits, target, lengths, power, reduction, gp, gw):
    from padertorch_amd import ops
    x = logits.detach().requires_grad_()
    pooled, weighted = ops.mask_bce_loss(x, target, lengths, power, reduction)
    total = (pooled * gp).sum()
    if weighted is not None:
        total = total + (weighted * gw).sum()
    grad, = torch.autograd.grad(total, x)
    return pooled.detach(), (None if weighted is None else weighted.detach()), grad


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_mask_loss.py needs an MI355X'
    dev = torch.device('cuda:0')
    torch.manual_seed(19)
    # the estimator's own view: out[..., :F] of a [C B, T, 2 F] buffer folded '(c b) t f -> b c t f'
    logits = (torch.randn(C * B, T, 2 * NF, device=dev) * 2).reshape(C, B, T, 2 * NF).transpose(0, 1)[..., :NF]
    target = torch.rand(B, C, T, NF, device=dev)
    stft = torch.randn(B, C, T, NF, dtype=torch.complex64, device=dev)
    gp, gw = torch.randn(B, device=dev), torch.randn(B, device=dev)
    lengths = torch.tensor(FRAMES, dtype=torch.int32, device=dev)
    valid, total = C * NF * sum(FRAMES), B * C * T * NF
    lines = [f'mask loss, forward + backward: B {B}, C {C}, T {T}, F {NF}, num_frames {FRAMES} ({valid} of {total} elements valid); '
             f'logits as the estimator\'s strided view; hip = ops.mask_bce_loss, library = the torch composition of the reference\'s loop']
    for reduction in ('mean', 'median'):
        for power in (None, stft):
            name = f'{reduction}, {"complex power" if power is not None else "no power"}'
            got, want = hip_step(logits, target, lengths, power, reduction, gp, gw), library_step(logits, target, power, reduction, gp, gw)
            diffs = [float(((a - b).abs().max() / b.abs().max()).cpu()) for a, b in zip(got, want) if a is not None]
            nbytes = 2 * valid * (8 + (8 if power is not None else 0)) + 4 * total

            def extra(res, nbytes=nbytes, diffs=diffs):
                gbs = nbytes / (res['hip']['median_us'] * 1e-6) / 1e9
                return dict(algorithmic_bytes=nbytes, achieved_GBs=round(gbs, 1), share_of_hbm_peak=round(gbs / HBM_GBS, 4),
                            library_over_hip=round(res['library']['median_us'] / res['hip']['median_us'], 2),
                            max_relative_difference=dict(zip(('pooled', 'weighted', 'd_logits') if len(diffs) == 3
                                                             else ('pooled', 'd_logits'), [float(f'{d:.2e}') for d in diffs])))
            lines.append(measure(name, dict(hip=lambda p=power, r=reduction: hip_step(logits, target, lengths, p, r, gp, gw),
                                            library=lambda p=power, r=reduction: library_step(logits, target, p, r, gp, gw)),
                                 args, extra))
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
