"""Restatement of BigVGAN's anti-aliased activation in plain torch ops, dtype-generic (fp32 / fp64, any device): the yardstick for shapes
tests/golden/g21_anti_alias.npz does not hold, and the unfused formulation scripts/bench_anti_alias.py times.

Written from the operator's definition (include/ptmi.h, "anti-aliased periodic activation"), with the clamps as index gathers:

    up     u[n] = r sum_j x[clamp(j - p, 0, T-1)] f[n + pl - j r],  n in [0, r T);  p = k // r - 1,  pl = p r + (k - r) // 2
    act    a(u) = u + sin^2(alpha' u) / (beta' + 1e-9)          (the 1e-9 added in the dtype of the parameter)
    down   y[m] = sum_i g[i] a[clamp(m d + i - left, 0, U-1)],  left = k // 2 - (k even);  without padding: no clamp, left = 0
"""
import torch
import torch.nn.functional as F


def upsample(x, f, ratio):
    """``x [B, C, T]``, ``f [k]`` -> ``[B, C, ratio T]``."""
    C, T, k = x.shape[1], x.shape[2], f.numel()
    p = k // ratio - 1
    pl = p * ratio + (k - ratio) // 2
    idx = (torch.arange(T + 2 * p, device=x.device) - p).clamp(0, T - 1)
    full = F.conv_transpose1d(x[..., idx], f.to(x.dtype).view(1, 1, k).expand(C, 1, k), stride=ratio, groups=C)
    return ratio * full[..., pl:pl + ratio * T]


def snake(u, alpha, beta=None, logscale=False):
    """``alpha`` / ``beta [C]`` (``beta=None``: the same parameter)."""
    a = alpha.view(1, -1, 1)
    b = a if beta is None else beta.view(1, -1, 1)
    if logscale:
        a, b = torch.exp(a), torch.exp(b)
    return u + (1.0 / (b + 1e-9)) * torch.sin(u * a) ** 2


def lowpass(a, g, stride, padding=True):
    """``a [B, C, U]``, ``g [k]`` -> ``[B, C, ceil(U / stride)]`` (padded) or ``[B, C, (U - k) // stride + 1]``."""
    C, U, k = a.shape[1], a.shape[2], g.numel()
    if padding:
        left, right = k // 2 - (1 if k % 2 == 0 else 0), k // 2
        idx = torch.arange(-left, U + right, device=a.device).clamp(0, U - 1)
        a = a[..., idx]
    return F.conv1d(a, g.to(a.dtype).view(1, 1, k).expand(C, 1, k), stride=stride, groups=C)


def activation1d(x, alpha, beta, up_filter, down_filter, up_ratio=2, down_ratio=2, logscale=False, act=None):
    """The whole operator; ``act``: a callable in place of Snake (``alpha`` / ``beta`` unused then)."""
    u = upsample(x, up_filter.reshape(-1), up_ratio)
    a = snake(u, alpha, beta, logscale) if act is None else act(u)
    return lowpass(a, down_filter.reshape(-1), down_ratio)


def run(x, alpha, beta, up_filter, down_filter, w, up_ratio=2, down_ratio=2, logscale=False, dtype=torch.float64):
    """Forward and the gradients of ``sum(y w)`` in ``dtype``: ``dict(y, dx, dalpha, dbeta)`` (``dbeta`` None for a shared parameter)."""
    x = x.detach().to(dtype).requires_grad_(True)
    alpha = alpha.detach().to(dtype).requires_grad_(True)
    beta = None if beta is None else beta.detach().to(dtype).requires_grad_(True)
    y = activation1d(x, alpha, beta, up_filter.to(dtype), down_filter.to(dtype), up_ratio, down_ratio, logscale)
    (y * w.to(dtype)).sum().backward()
    return dict(y=y.detach(), dx=x.grad, dalpha=alpha.grad, dbeta=None if beta is None else beta.grad)


_GOLDEN = None


def golden():
    """tests/golden/g21_anti_alias.npz (loaded once; ``cases`` decoded)."""
    global _GOLDEN
    if _GOLDEN is None:
        import json
        from pathlib import Path

        import numpy as np
        d = dict(np.load(Path(__file__).resolve().parent / 'golden' / 'g21_anti_alias.npz', allow_pickle=False))
        for key in ('cases', 'keys_snake', 'keys_snakebeta'):
            d[key] = json.loads(str(d[key]))
        _GOLDEN = d
    return _GOLDEN


def activation_cases():
    """Names of the golden cases that are a whole Activation1d (the others are the stand-alone resamplers)."""
    return [n for n, c in golden()['cases'].items() if c['cls'] in ('Snake', 'SnakeBeta')]


def case_tensors(name):
    """``(meta, dict of torch tensors)`` of a golden case."""
    g = golden()
    pre = name + '_'
    return g['cases'][name], {k[len(pre):]: torch.from_numpy(v) for k, v in g.items()
                              if k.startswith(pre) and getattr(v, 'ndim', 0) > 0}


def gate(dev32):
    """The tolerance of a quantity relative to its largest fp64 value: four times the reference's own fp32 deviation (another summation
    order over the taps and another sine are each an fp32 rounding of that size), at least four roundings of the largest value."""
    return max(4 * float(dev32), 4 * 2.0 ** -23)


def rel_dev(got, want):
    """``max|got - want| / max|want|`` in fp64 (absolute where ``want`` is all zero)."""
    got, want = got.detach().double().cpu(), want.detach().double().cpu()
    assert got.shape == want.shape, (got.shape, want.shape)
    assert bool(torch.isfinite(got).all())
    scale = float(want.abs().max()) if want.numel() else 0.
    d = float((got - want).abs().max()) if want.numel() else 0.
    return d / scale if scale > 0 else d
