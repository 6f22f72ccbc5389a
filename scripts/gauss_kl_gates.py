"""The gates of tests/test_gpu_kl_divergence.py: the explicit formulas of DESIGN.md 3.5v (what csrc/gauss_kl.hip evaluates: kl and the
five gradients written out, no autograd) in fp32 on the CPU against that file's fp64 autograd restatement over the test's own cases; per
quantity the largest error relative to the largest magnitude of the quantity in the case, and four times it (two legitimate fp32
evaluations with different summation orders).  Also cond(T) per case and the restatement against torch.distributions.  No GPU needed.

    python scripts/gauss_kl_gates.py > profiles/gauss_kl_gates.txt
"""
import sys
from pathlib import Path

import torch
from torch.distributions import MultivariateNormal, kl_divergence

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from tests.test_gpu_kl_divergence import CASES, GATES, inputs, restatement  # noqa: E402


def formulas(mu, sigma, m, scale, G):
    """``(kl, dmu, dsigma, dm, dscale)`` by the explicit formulas, in the dtype of ``mu``."""
    D = mu.shape[1]
    diff = m[None] - mu[:, None]                                                    # [B, K, D]
    gs, s2 = G.sum(0), sigma * sigma
    if scale.dim() == 3:
        T = scale.tril()
        L = torch.linalg.solve_triangular(T, torch.eye(D, dtype=mu.dtype).expand_as(T), upper=False)
        c, diag = (L * L).sum(-2), torch.diagonal(T, dim1=1, dim2=2)
        y = torch.einsum('kid,bkd->bki', L, diff)
        kl = diag.log().sum(-1)[None] - sigma.log().sum(-1)[:, None] + 0.5 * (s2 @ c.T + (y * y).sum(-1) - D)
        z = torch.einsum('kid,bki->bkd', L, y)
        dL = torch.einsum('bk,bki,bkd->kid', G, y, diff) + L * (G.T @ s2)[:, None, :]
        dscale = -(L.transpose(1, 2) @ dL.tril() @ L.transpose(1, 2)).tril() + torch.diag_embed(gs[:, None] / diag)
    else:
        c = 1 / (scale * scale)
        kl = (scale.log()[None] - sigma.log()[:, None] + (s2[:, None] + diff * diff) * (0.5 * c)[None] - 0.5).sum(-1)
        z = diff * c[None]
        dscale = gs[:, None] / scale - c / scale * torch.einsum('bk,bkd->kd', G, s2[:, None] + diff * diff)
    dmu, dm = -torch.einsum('bk,bkd->bd', G, z), torch.einsum('bk,bkd->kd', G, z)
    dsigma = sigma * (G @ c) - G.sum(1, keepdim=True) / sigma
    return kl, dmu, dsigma, dm, dscale


worst = {full: dict.fromkeys(GATES[full], 0.) for full in GATES}
print('case (B, K, D, full)          kl        dmu       dsigma    dm        dscale    cond(T)   vs torch.distributions')
for case in CASES:
    B, K, D, full = case
    want = restatement(*inputs(B, K, D, full))
    got = formulas(*inputs(B, K, D, full, torch.float32))
    err = {k: float((a.double() - w).abs().max() / w.abs().max()) for k, a, w in zip(GATES[full], got, want)}
    for k in err:
        worst[full][k] = max(worst[full][k], err[k])
    mu, sigma, m, scale, _ = inputs(B, K, D, full)
    T = scale.tril() if full else torch.diag_embed(scale)
    ref = kl_divergence(MultivariateNormal(mu[:, None], scale_tril=torch.diag_embed(sigma)[:, None]), MultivariateNormal(m, scale_tril=T))
    print(f'{str(case):<30}' + ''.join(f'{err[k]:<10.1e}' for k in err) + f'{float(torch.linalg.cond(T).max()):<10.2f}'
          f'{float((want[0] - ref).abs().max() / ref.abs().max()):.1e}')
for full in GATES:
    print(f'\n{"full-covariance" if full else "diagonal"} prior: quantity   fp32 formulas vs fp64    gate (x 4)')
    for k, v in worst[full].items():
        print(f'{k:<16}{v:<28.3e}{4 * v:.1e}')
