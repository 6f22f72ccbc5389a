"""The gates of tests/test_gpu_cpc_contrast.py: that file's restatement of CPC1d.contrast + cross-entropy in fp32 on the CPU against its
fp64 run over the test's own cases; per quantity the largest error relative to the largest magnitude of the quantity in the case, and
four times it (two legitimate fp32 evaluations with different summation orders).  Also what the hit comparison excludes (rows whose fp64
top-two gap is below 1e-3 of the largest finite |logit|) and the reference's hit rate per case.  No GPU needed.

    python scripts/cpc_contrast_gates.py > profiles/cpc_contrast_gates.txt
"""
import math
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from tests.test_gpu_cpc_contrast import CASES, GATES, inputs, log_batch_mask, restatement  # noqa: E402

worst = dict.fromkeys(GATES, 0.)
print('case                                              ce        dz_hat    dz        logits    excluded  hit rate')
for case in CASES:
    mode, b, d, t, steps, dist, labels, invert, ratio = case
    runs = []
    for dt in (torch.float32, torch.float64):
        z_hat, z, gout = inputs(b, d, t, steps, dt)
        lbm = log_batch_mask(b, labels, invert, dt) if mode == 'batch' else None
        runs.append(restatement(z_hat, z, gout, mode, steps, dist, lbm, ratio))
    (got, got_dzh, got_dz), (want, want_dzh, want_dz) = runs
    top = max(float(w[0][w[0] > -math.inf].abs().max()) for w in want)
    ce_top = max(float(w[1].abs().max()) for w in want)
    err = {'ce': max(float((a[1].double() - w[1]).abs().max()) for a, w in zip(got, want)) / ce_top,
           'dz_hat': float((got_dzh.double() - want_dzh).abs().max() / want_dzh.abs().max()),
           'dz': float((got_dz.double() - want_dz).abs().max() / want_dz.abs().max()),
           'logits': max(float((a[0].double() - w[0])[w[0] > -math.inf].abs().max()) for a, w in zip(got, want)) / top}
    rows = excluded = hits = 0
    for logits, _, h, _ in want:
        top2 = torch.topk(logits, 2, dim=1).values
        rows, hits = rows + h.numel(), hits + float(h.sum())
        excluded += int((top2[:, 0] - top2[:, 1] < 1e-3 * top).sum())
    for k in worst:
        worst[k] = max(worst[k], err[k])
    name = f'{mode} b={b} d={d} t={t} steps={steps} dist={dist} r={ratio}'
    print(f'{name:<50}' + ''.join(f'{err[k]:<10.1e}' for k in GATES) + f'{excluded / rows:<10.3f}{hits / rows:.3f}')
print('\nquantity        fp32 restatement vs fp64    gate (x 4)')
for k, v in worst.items():
    print(f'{k:<16}{v:<28.3e}{4 * v:.1e}')
