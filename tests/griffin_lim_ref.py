"""fp64 numpy restatement of fast Griffin-Lim (padertorch/contrib/mk/synthesis/parametric/griffin_lim.py:32-156) on
``oracle.stft_np.stft`` / ``istft``.  A helper of the Griffin-Lim tests (not a conftest): the golden ``g20_griffin_lim.npz`` pins it to
the reference (test_griffin_lim_host.py), and GPU tests may use it where the golden holds no answer."""
import json
from pathlib import Path

import numpy as np

from oracle import stft_np

GOLDEN = Path(__file__).resolve().parent / 'golden' / 'g20_griffin_lim.npz'
CASES = ('s64', 's512', 's40', 's512w')
_cache = {}


def golden():
    """The golden file, loaded once and shared (read-only by convention)."""
    if 'g' not in _cache:
        d = dict(np.load(GOLDEN, allow_pickle=False))
        d['geometries'] = json.loads(str(d['geometries']))
        _cache['g'] = d
    return _cache['g']


def stft_kwargs(geometry):
    return {k: v for k, v in geometry.items() if k in ('size', 'shift', 'window', 'window_length', 'fading')}


def project(a, y):
    """``a exp(j angle(y))`` with ``angle(0) = 0``."""
    return a * np.exp(1j * np.angle(y))


def step(a, y, **kw):
    """``griffin_lim_step``: ``(STFT(iSTFT(P)), audio)``."""
    audio = stft_np.istft(project(a, y), **kw)
    return stft_np.stft(audio, **kw), audio


def fast_griffin_lim(a, x0, alpha=0.95, iterations=100, atol=0.1, **kw):
    """Returns ``(signal, xs, rmse)``: ``xs[n]`` / ``rmse[n]`` behind iteration n (those that ran)."""
    a = np.asarray(a, dtype=np.float64)
    x = project(a, np.asarray(x0, dtype=np.complex128))
    y = x
    xs, rmse = [], []
    for _ in range(iterations):
        x_, _audio = step(a, y, **kw)
        y = x_ + alpha * (x_ - x)
        x = x_
        xs.append(x)
        rmse.append(np.sqrt(np.mean((np.abs(x) - a) ** 2)))
        if rmse[-1] < atol:
            break
    return stft_np.istft(project(a, x), **kw), xs, np.array(rmse)
