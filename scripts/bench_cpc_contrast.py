"""The fused CPC contrast (forward + backward) against the reference's formulation composed from torch ops on the device, at b = 16,
d = 256, t = 500, steps (-20, -10, 10, 20), for each negatives mode: time per call (median and spread of the repeats after a warm-up,
host clock around a synchronise) and peak allocated memory.

    python scripts/bench_cpc_contrast.py >> profiles/cpc_contrast.txt
"""
import sys
import time
from pathlib import Path

import torch
import torch.nn.functional as F

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from padertorch_amd.ops.cpc_contrast import contrastive_scores  # noqa: E402

B, D, T, STEPS, DIST, TEMP = 16, 256, 500, (-20, -10, 10, 20), 10, 0.1


def composed(z_hat, z, mode):
    """contrastive.py:343-471 + CrossEntropyLoss, dense."""
    loss = 0.
    for n, s in enumerate(STEPS):
        Ts, qoff, sh = T - abs(s), max(-s, 0), max(s, 0)
        q = z_hat[:, n * D:(n + 1) * D, qoff:qoff + Ts].transpose(1, 2)
        band = (torch.arange(T, device=z.device)[:, None] - torch.arange(Ts, device=z.device)[None]).abs()
        logmask = torch.log(1. - ((band <= DIST - 1) & (band > 0)).float())
        if mode == 'batch':
            logits = torch.matmul(q.transpose(0, 1), z[:, :, sh:sh + Ts].permute(2, 1, 0)).permute(1, 2, 0) / TEMP
            targets = torch.arange(B, device=z.device)[:, None].expand(B, Ts)
        elif mode == 'time':
            logits = torch.matmul(q, torch.roll(z, -sh, 2)).transpose(1, 2) / TEMP + logmask
            targets = torch.arange(Ts, device=z.device)[None].expand(B, Ts)
        else:
            keys = torch.roll(z, -sh, 2).permute(1, 0, 2).reshape(D, B * T)
            logits = (torch.matmul(q, keys).transpose(1, 2) / TEMP).view(B, B, T, Ts)
            logits = (logits + torch.eye(B, device=z.device)[:, :, None, None] * logmask.nan_to_num(neginf=-1e30)).view(B, B * T, Ts)
            targets = torch.arange(B, device=z.device)[:, None] * T + torch.arange(Ts, device=z.device)[None]
        loss = loss + F.cross_entropy(logits, targets)
    return loss


def fused(z_hat, z, mode):
    return sum(st.ce.mean() for st in contrastive_scores(z_hat, z, STEPS, mode, TEMP, DIST))


def measure(fn, mode, warmup=5, repeats=20):
    z = torch.randn(B, D, T, device='cuda', requires_grad=True)
    z_hat = torch.randn(B, len(STEPS) * D, T, device='cuda', requires_grad=True)
    times = []
    for i in range(warmup + repeats):
        if i == warmup:
            torch.cuda.reset_peak_memory_stats()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        torch.autograd.grad(fn(z_hat, z, mode), (z_hat, z))
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    times = sorted(times[warmup:])
    return times[len(times) // 2] * 1e3, times[0] * 1e3, times[-1] * 1e3, torch.cuda.max_memory_allocated() / 2 ** 20


if __name__ == '__main__':
    print(f'b = {B}, d = {D}, t = {T}, steps {STEPS}, dist {DIST}; forward + backward, ms median (min .. max), peak allocated MiB')
    for mode in ('time', 'all', 'batch'):
        for name, fn in (('fused', fused), ('composed torch ops', composed)):
            med, lo, hi, mem = measure(fn, mode)
            print(f'{mode:<6} {name:<20} {med:8.3f} ({lo:.3f} .. {hi:.3f})   {mem:8.1f} MiB')
