"""One training-mode forward of NormalizedLogMelExtractor at the audio-tagging shape (the reference model's settings: 44.1 kHz, STFT 2048,
shift 882, 128 filters, frequency warping, one time and one frequency mask; 16 examples of 10 s) against the same stages composed from
torch ops on the device - the reference's code path: a materialised per-example filterbank, a batched vector-matrix product, masks built
on the host.  Both paths draw on the host; alternating, host clock around a device synchronise.  Results: profiles/je_features.txt.

    python scripts/bench_je_features.py
"""
import sys
import time
from pathlib import Path

import numpy as np
import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from padertorch_amd.contrib.je.modules.features import NormalizedLogMelExtractor, _mel2hz  # noqa: E402
from padertorch_amd.contrib.je.modules.augment import Mask  # noqa: E402

B, T, RATE, SIZE, M = 16, 500, 44100, 2048, 128
F = SIZE // 2 + 1


def warp(edges):
    a = np.random.uniform(.85, 1.15, (len(edges), 1, 1, 1))
    lo, hi = edges[..., :1], edges[..., -1:]
    knee = lo + .7 * (hi - lo)
    low = lo + a * (edges - lo)
    high = hi - (hi - edges) * (hi - (lo + a * (knee - lo))) / (hi - knee)
    return np.where(edges <= knee, low, high)


ext = NormalizedLogMelExtractor(RATE, SIZE, M, frequency_warping_fn=warp, n_time_masks=1, n_frequency_masks=1).cuda().train()
tm, fm = Mask(-1, 1, 70, 1.), Mask(-2, 1, 20, 1.)
state = dict(n=torch.zeros(1, 1, M, 1, device='cuda'), mean=torch.zeros(1, 1, M, 1, device='cuda'), power=torch.ones(1, 1, M, 1, device='cuda'))


def torch_path(x, seq_len):
    """features.py:142-206 with the reference's ops: materialised per-example filterbank, batched vector-matrix product, ..."""
    hz = ext.warped_edges_hz(B).astype(np.float64)
    f = np.arange(F) * (RATE / SIZE)
    l, c, r = hz[:, :-2, None], hz[:, 1:-1, None], hz[:, 2:, None]
    fb = np.clip(np.minimum((f - l) / (c - l), (r - f) / (r - c)), 0, None).astype(np.float32)
    fb = fb / (fb.sum(-1, keepdims=True) + 1e-6)
    fb = torch.from_numpy(fb[:, None, None]).transpose(-2, -1).to(x.device)             # [B, 1, 1, F, M]
    p = torch.sum(x ** 2, dim=-1)
    y = torch.log(p[..., None, :].matmul(fb).squeeze(-2) + 1e-12).transpose(-2, -1)
    mask = (torch.arange(T, device=x.device) < torch.as_tensor(seq_len, device=x.device)[:, None, None, None]).float()
    n = mask.sum((0, 3), keepdim=True)
    mean, power = (y * mask).sum((0, 3), keepdim=True) / n, (y * y * mask).sum((0, 3), keepdim=True) / n
    state['n'] += n
    keep = 1 - n / state['n']
    state['mean'].mul_(keep).add_((1 - keep) * mean)
    state['power'].mul_(keep).add_((1 - keep) * power)
    nn = state['n'].clamp(min=2)
    var = (state['power'] * (nn / (nn - 1)) - state['mean'] ** 2).clamp(min=0) + 1e-5
    y = torch.clamp((y - state['mean']) * torch.rsqrt(var + 1e-5) * mask, -6, 6)
    for m, axis, sl in ((tm, 3, seq_len), (fm, 2, None)):
        on, off = m.draw(B, y.shape[axis], sl)
        idx = torch.arange(y.shape[axis]).float()[(...,) + (3 - axis) * (None,)].expand(y.shape)
        on, off = (torch.from_numpy(v[0]).float()[:, None, None, None] for v in (on, off))
        y = y * ((idx < on) + (idx >= off)).float().to(y.device)
    return y


x = torch.randn(B, 1, T, F, 2, device='cuda')
seq_len = [T - 7 * b for b in range(B)]
paths = {'hip': lambda: ext(x, seq_len)[0], 'torch': lambda: torch_path(x, seq_len)}
np.random.seed(0); torch.manual_seed(0); a = paths['hip']()          # noqa: E702
np.random.seed(0); torch.manual_seed(0); b = paths['torch']()        # noqa: E702
print('max |hip - torch| on the same draws:', float((a - b).abs().max()))
times = {k: [] for k in paths}
for it in range(25):
    for k, fn in paths.items():                                      # alternating
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        if it >= 5:
            times[k].append((time.perf_counter() - t0) * 1e3)
for k, v in times.items():
    v = np.sort(v)
    print(f'{k}: median {np.median(v):.3f} ms, min {v[0]:.3f}, max {v[-1]:.3f} over {len(v)} forwards (B={B}, T={T}, F={F}, M={M})')
