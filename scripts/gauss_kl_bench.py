"""gaussian_kl_divergence (csrc/gauss_kl.hip) against the reference's formulation (padertorch/ops/losses/kl_divergence.py:17-60) composed
from torch ops on the same device, for one shape and both prior kinds: forward and forward + backward, time per call (median and spread
of the repeats after a warm-up, host clock around a synchronise) and peak allocated memory above the inputs.  Also the launches of one
fused forward + backward as `_lib.KERNEL_TIMERS` sees them.

    python scripts/gauss_kl_bench.py B K D >> profiles/gauss_kl_times.txt
"""
import sys
import time
from pathlib import Path

import torch
from torch.distributions import MultivariateNormal, Normal
from torch.distributions import kl_divergence as kld

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from padertorch_amd import _lib  # noqa: E402
from padertorch_amd.ops import gaussian_kl_divergence  # noqa: E402


def composed(q, p):
    """kl_divergence.py:27-60."""
    D = q.loc.shape[-1]
    p_loc = p.loc.contiguous().view(-1, D)
    if isinstance(p, MultivariateNormal):
        p_scale_tril = p.scale_tril.contiguous().view(-1, D, D)
        q_loc, q_scale = q.loc.contiguous().view(-1, D), q.scale.contiguous().view(-1, D)
        term1 = torch.diagonal(p_scale_tril, dim1=1, dim2=2).log().sum(-1)[:, None] - q_scale.log().sum(-1)
        L = p_scale_tril.inverse()
        term2 = (L.pow(2).sum(-2)[:, None, :] * q_scale.pow(2)).sum(-1)
        term3 = ((p_loc[:, None, :] - q_loc) @ L.transpose(1, 2)).pow(2.0).sum(-1)
        return (term1 + 0.5 * (term2 + term3 - D)).transpose(0, 1)
    q_loc, q_scale = q.loc.contiguous().view(-1, 1, D), q.scale.contiguous().view(-1, 1, D)
    return kld(Normal(q_loc, q_scale, validate_args=False), Normal(p_loc, p.scale.contiguous().view(-1, D), validate_args=False)).sum(-1)


def measure(fn, params, full, backward, warmup=5, repeats=30):
    mu, sigma, m, scale = params
    times, base = [], 0
    for i in range(warmup + repeats):
        if i == warmup:
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        p = MultivariateNormal(m, scale_tril=scale, validate_args=False) if full else Normal(m, scale, validate_args=False)
        kl = fn(Normal(mu, sigma, validate_args=False), p)
        if backward:
            torch.autograd.grad(kl.mean(), params)
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
        del kl, p
    times = sorted(times[warmup:])
    return times[len(times) // 2] * 1e3, times[0] * 1e3, times[-1] * 1e3, (torch.cuda.max_memory_allocated() - base) / 2 ** 20


if __name__ == '__main__':
    B, K, D = (int(v) for v in sys.argv[1:4])
    print(f'B = {B}, K = {K}, D = {D}; ms median (min .. max), peak allocated MiB above the inputs')
    for full in (True, False):
        g = torch.Generator().manual_seed(0)
        mu, m, sigma = torch.randn(B, D, generator=g), torch.randn(K, D, generator=g), 0.2 + torch.rand(B, D, generator=g)
        scale = 0.5 + torch.rand(K, D, generator=g)
        if full:
            scale = torch.diag_embed(scale) + 0.5 * torch.tril(torch.randn(K, D, D, generator=g), -1) / D ** 0.5
        params = [x.cuda().requires_grad_(True) for x in (mu, sigma, m, scale)]
        for backward in (False, True):
            for name, fn in (('fused', gaussian_kl_divergence), ('composed torch ops', composed)):
                med, lo, hi, mem = measure(fn, params, full, backward)
                print(f'{"full" if full else "diag"}  {"fwd+bwd" if backward else "fwd    "}  {name:<20} {med:8.3f} ({lo:.3f} .. {hi:.3f})   '
                      f'{mem:8.1f} MiB')
        _lib.KERNEL_TIMERS = []
        kl = gaussian_kl_divergence(Normal(params[0], params[1], validate_args=False),
                                    MultivariateNormal(params[2], scale_tril=params[3], validate_args=False) if full
                                    else Normal(params[2], params[3], validate_args=False))
        torch.autograd.grad(kl.mean(), params)
        torch.cuda.synchronize()
        print('      launches: ' + ', '.join(f'{n} {a.elapsed_time(b) * 1e3:.0f} us' for n, a, b in _lib.KERNEL_TIMERS))
        _lib.KERNEL_TIMERS = None
