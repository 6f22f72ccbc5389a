"""Cases of the clip + Adam gates: inputs, segment layouts, the fp64 restatement's results and the gates derived from its own fp32 run.
Shared by tests/test_oracle_optim.py (CPU: the restatement against torch, the input condition) and tests/test_gpu_optim_paths.py (the
kernels of csrc/optim.hip against the restatement).  Nothing here touches a GPU.
"""
import itertools

import numpy as np

from oracle import optim_np

HYPER = dict(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8)
MAX_NORM = 0.5
ZEROS = 100                       # leading elements with g = m = v = 0
EPS32 = 2.0 ** -24
CAP = 2.0 ** -17                  # the input condition: no dev32 above it (test_oracle_optim.py)
QUANTITIES = ('p', 'm', 'v')

#: (t, weight decay, clipped)
FULL = list(itertools.product((1, 2, 1000, 100000), (0.0, 0.01), (False, True)))
PAIR = [(2, 0.01, True), (1, 0.0, False)]

BIG_N = 8192 * 1024 + 5 * 1024 + 3          # 8 393 731: five workgroups take a second trip of the grid-stride loop, partial tail
BIG_SPLIT = 8_389_123                       # odd, inside the second trip


def _cycle(values, count):
    return [values[i % len(values)] for i in range(count)]


def _max_layout(nseg):
    lengths = [1 + i % 7 for i in range(nseg)]
    lengths[nseg // 2 - 12] = 20_001          # the long remainder, off the middle: the search ends on either side of it
    return [(n, 0) for n in lengths]


#: name -> [(elements, misalignment of the parameter's address in floats)], in flat order
LAYOUTS = {
    'one-0': [(5120, 0)],
    'one-1': [(5121, 0)],
    'one-3': [(66_563, 0)],
    'odd': [(n, 0) for n in _cycle((1, 2, 3, 5, 7, 4, 257, 6), 8 * 40)],
    'max': _max_layout(1024),
    'offset': [(300 + (7 * i) % 11, 1 + i % 3) for i in range(24)],
    'empty': [(0, 0), (300, 0), (0, 0), (0, 0), (517, 0), (1234, 0), (0, 0)],
    'big': [(BIG_SPLIT, 0), (BIG_N - BIG_SPLIT, 0)],
}
TOO_MANY = _max_layout(1025)
SMALL = ('one-0', 'one-1', 'one-3', 'odd', 'offset')

CASES = [(name, *c) for name in SMALL for c in FULL] + [(name, *c) for name in ('max', 'empty', 'big') for c in PAIR]


def case_id(case):
    name, t, wd, clipped = case
    return f'{name}-t{t}-wd{wd:g}-{"clip" if clipped else "noclip"}'


def size(name):
    return sum(n for n, _ in LAYOUTS[name])


def flat_offsets(layout):
    return np.concatenate([[0], np.cumsum([n for n, _ in layout])]).astype(np.int64)


#: seeds other than the default, per (n, t): where a draw misses CAP it gets another seed, never another cap
SEEDS = {}
_INPUTS, _REFS = {}, {}


def inputs(n, t):
    """``dict(p, g, m, v)`` in fp32: gradients over ten decades, moments of their size (none before the first step)."""
    key = (n, t)
    if key not in _INPUTS:
        rng = np.random.default_rng(SEEDS.get(key, (n, t)))
        mag = 10.0 ** rng.uniform(-8, 2, n)
        g = rng.standard_normal(n) * mag
        p = rng.standard_normal(n)
        if t == 1:
            m, v = np.zeros(n), np.zeros(n)
        else:
            m = 0.3 * rng.standard_normal(n) * mag
            v = 0.5 * (rng.standard_normal(n) * mag) ** 2
        for a in (g, m, v):
            a[:ZEROS] = 0
        _INPUTS[key] = {k: a.astype(np.float32) for k, a in dict(p=p, g=g, m=m, v=v).items()}
    return _INPUTS[key]


#: the wrapper's test at the segment limit compares with torch.optim.Adam in fp32 on the CPU at the tolerances of test_gpu_optim.py.
#: That reference is only as good as its own fp32 arithmetic: the draws are ones on which it stays within a quarter of the tolerance of
#: the fp64 restatement (test_oracle_optim.py).  (The draw of seed 1024 holds an element whose clipped gradient and weight decay cancel
#: to 3e-8 at t = 1, next to eps = 1e-8: torch's own fp32 step is 6.6e-6 off there.)
WRAPPER = dict(lr=1e-3, weight_decay=0.01, max_norm=0.5, rtol=2e-6, atol=2e-7, steps=3)
WRAPPER_SEEDS = {1024: 11024, 1025: 1025}


def wrapper_draw(count):
    """``count`` parameters of one to three elements and their gradients of three steps (torch, CPU, fp32)."""
    import torch
    gen = torch.Generator().manual_seed(WRAPPER_SEEDS[count])
    params = [torch.randn(1 + i % 3, generator=gen) for i in range(count)]
    grads = [[torch.randn(p.shape, generator=gen) * (0.1 if step % 2 else 3.0) for p in params] for step in range(WRAPPER['steps'])]
    return params, grads


def deviation(got, r64):
    """Per quantity: ``max_i |q_i - q64_i| / terms_q,i`` over every element."""
    return {q: optim_np.scaled_error(got[q], r64[q], r64['terms'][q]) for q in QUANTITIES}


def gates(dev32, clipped):
    """``max(4 dev32, 4 * 2^-24)``: another order of fp32 operations (fused multiply-adds against separate roundings).  A clipped step
    takes its coefficient from the kernel's own fp32 norm, which test_grad_norm_vs_fp64 holds to 2e-7: the gradient enters m and p
    once and v squared."""
    extra = dict(p=2e-7, m=2e-7, v=4e-7) if clipped else dict(p=0.0, m=0.0, v=0.0)
    return {q: max(4 * dev32[q], 4 * EPS32) + extra[q] for q in QUANTITIES}


def reference(n, t, wd, clipped, **hyper):
    """``(inputs, fp64 run, dev32, gates)`` of one step, computed once.  ``hyper`` replaces entries of ``HYPER`` / ``max_norm``."""
    key = (n, t, wd, clipped, tuple(sorted(hyper.items())))
    if key not in _REFS:
        x = inputs(n, t)
        kw = dict(HYPER, weight_decay=wd, max_norm=MAX_NORM if clipped else None)
        kw.update(hyper)
        r64 = optim_np.clip_adam_step(x['p'], x['g'], x['m'], x['v'], t, **kw)
        r32 = optim_np.clip_adam_step(x['p'], x['g'], x['m'], x['v'], t, dtype=np.float32, **kw)
        assert all(r32[q].dtype == np.float32 and r64[q].dtype == np.float64 for q in QUANTITIES)
        dev32 = deviation(r32, r64)
        _REFS[key] = (x, r64, dev32, gates(dev32, clipped))
    return _REFS[key]
