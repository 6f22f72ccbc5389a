"""The clip + Adam restatement (oracle/optim_np.py) against torch's own float64 step, and the input condition of the GPU gates
(tests/test_gpu_optim_paths.py): on every input those gates use, the restatement's float32 run stays within 2^-17 of its float64 run."""
import numpy as np
import pytest
import torch

import optim_paths_ref as R
from oracle import optim_np


def torch_step(x, t, wd, max_norm, shapes):
    """clip_grad_norm_ + torch.optim.Adam(foreach=False) in float64 on parameters of ``shapes`` cut from the flat inputs."""
    cut, off = [], 0
    for s in shapes:
        n = int(np.prod(s))
        cut.append((off, n, s))
        off += n
    assert off == x['p'].size
    take = lambda a, o, n, s: torch.from_numpy(np.asarray(a[o:o + n], np.float64).reshape(s).copy())    # noqa: E731
    params = [torch.nn.Parameter(take(x['p'], *c)) for c in cut]
    opt = torch.optim.Adam(params, lr=R.HYPER['lr'], betas=(R.HYPER['beta1'], R.HYPER['beta2']), eps=R.HYPER['eps'], weight_decay=wd,
                           foreach=False)
    for P, c in zip(params, cut):
        P.grad = take(x['g'], *c)
        opt.state[P] = {'step': torch.tensor(float(t - 1)), 'exp_avg': take(x['m'], *c), 'exp_avg_sq': take(x['v'], *c)}
    norm = None
    if max_norm is not None:
        norm = float(torch.nn.utils.clip_grad_norm_(params, max_norm))
    opt.step()
    assert all(float(opt.state[P]['step']) == t for P in params)
    flat = lambda ts: np.concatenate([a.detach().numpy().reshape(-1) for a in ts])                      # noqa: E731
    return dict(p=flat(params), m=flat([opt.state[P]['exp_avg'] for P in params]),
                v=flat([opt.state[P]['exp_avg_sq'] for P in params]), norm=norm)


@pytest.mark.parametrize('clipped', [False, True], ids=['noclip', 'clip'])
@pytest.mark.parametrize('wd', [0.0, 0.01])
@pytest.mark.parametrize('t', [1, 2, 1000])
def test_float64_run_is_torch_adam_after_clip_grad_norm(t, wd, clipped):
    shapes = [(48, 257), (48,), (3, 5, 7), (1,), (514, 3), (6,)]
    x = R.inputs(sum(int(np.prod(s)) for s in shapes), t)
    max_norm = R.MAX_NORM if clipped else None
    want = torch_step(x, t, wd, max_norm, shapes)
    got = optim_np.clip_adam_step(x['p'], x['g'], x['m'], x['v'], t, weight_decay=wd, max_norm=max_norm, **R.HYPER)
    if clipped:
        assert abs(got['norm'] - want['norm']) <= 1e-12 * want['norm']
        assert got['clip'] < 1          # the case does clip
    else:
        assert got['clip'] == 1
    for q, e in R.deviation(want, got).items():
        assert e <= 1e-12, (q, e)
    assert not np.array_equal(got['p'], x['p'].astype(np.float64))


def test_scaled_error_counts_what_nothing_enters_as_exact_or_wrong():
    one = np.ones(3)
    assert optim_np.scaled_error([1., 0., 2.], [1., 0., 3.], [1., 0., 4.]) == 0.25
    assert optim_np.scaled_error([1., 1e-30, 2.], [1., 0., 2.], [1., 0., 4.]) == np.inf
    assert optim_np.scaled_error([1., np.nan, 2.], one, one) == np.inf
    assert optim_np.scaled_error([], [], []) == 0.0


def test_float32_run_rounds_the_norm_once_and_clips_in_float32():
    x = R.inputs(R.size('odd'), 2)
    r32 = optim_np.clip_adam_step(x['p'], x['g'], x['m'], x['v'], 2, weight_decay=0.01, max_norm=R.MAX_NORM, dtype=np.float32, **R.HYPER)
    norm64 = float(np.sqrt(np.square(x['g'].astype(np.float64)).sum()))
    assert r32['norm'] == norm64
    assert r32['clip'] == np.float32(R.MAX_NORM) / (np.float32(norm64) + np.float32(1e-6)) and type(r32['clip']) is np.float32
    assert all(r32[q].dtype == np.float32 for q in R.QUANTITIES)


@pytest.mark.parametrize('case', R.CASES, ids=R.case_id)
def test_input_condition_of_the_gpu_gates(case):
    """dev32 <= 2^-17 for p, m and v on every (size, t, weight decay, clip) the GPU gates run at: the gates are then at most 2^-15."""
    name, t, wd, clipped = case
    _, r64, dev32, gate = R.reference(R.size(name), t, wd, clipped)
    print(f'{R.case_id(case):34s} dev32 ' + '  '.join(f'{q} {dev32[q] / R.EPS32:6.2f} x 2^-24' for q in R.QUANTITIES))
    assert all(np.isfinite(r64[q]).all() for q in R.QUANTITIES)
    assert clipped == (r64['clip'] < 1)
    for q in R.QUANTITIES:
        assert dev32[q] <= R.CAP, (q, dev32[q] / R.EPS32)
        assert gate[q] >= 4 * R.EPS32


@pytest.mark.parametrize('count', sorted(R.WRAPPER_SEEDS))
def test_wrapper_draws_keep_torch_float32_within_a_quarter_of_the_tolerance(count):
    """The wrapper's GPU test compares with torch's fp32 step on the CPU: on its draws that step is within a quarter of the tolerance of
    three fp64 steps of the restatement."""
    W = R.WRAPPER
    init, grads = R.wrapper_draw(count)
    cpu = [torch.nn.Parameter(p.clone()) for p in init]
    ref = torch.optim.Adam(cpu, lr=W['lr'], weight_decay=W['weight_decay'], foreach=False)
    cat = lambda ts: torch.cat([a.detach().reshape(-1) for a in ts]).numpy()                                # noqa: E731
    p = cat(cpu).astype(np.float64)
    m, v = np.zeros_like(p), np.zeros_like(p)
    for step, gs in enumerate(grads):
        for P, g in zip(cpu, gs):
            P.grad = g.clone()
        torch.nn.utils.clip_grad_norm_(cpu, W['max_norm'])
        ref.step()
        r = optim_np.clip_adam_step(p, cat(gs), m, v, step + 1, lr=W['lr'], weight_decay=W['weight_decay'], max_norm=W['max_norm'],
                                    **{k: R.HYPER[k] for k in ('beta1', 'beta2', 'eps')})
        p, m, v = r['p'], r['m'], r['v']
        worst = (np.abs(cat(cpu) - p) / (W['atol'] + W['rtol'] * np.abs(p))).max()
        print(f'{count} parameters, step {step + 1}: torch fp32 uses {worst:.3f} of the tolerance')
        assert worst <= 0.25


def test_layouts_reach_what_they_are_for():
    off = {k: R.flat_offsets(v) for k, v in R.LAYOUTS.items()}
    assert {R.size(k) % 4 for k in ('one-0', 'one-1', 'one-3')} == {0, 1, 3}
    assert all(1000 <= R.size(k) <= 70_000 for k in R.LAYOUTS if k != 'big')
    # 'odd': some group of four flat elements holds three segments
    o = off['odd']
    assert any(np.searchsorted(o, 4 * q + 3, 'right') - np.searchsorted(o, 4 * q, 'right') >= 2 for q in range(R.size('odd') // 4))
    assert len(R.LAYOUTS['max']) == 1024 and len(R.TOO_MANY) == 1025
    # 'offset': every parameter starts 1, 2 or 3 floats into its allocation; flat offsets both = 0 and != 0 (mod 4); misalignments of
    # pointer and flat offset that cancel (aligned whole-group accesses) and that do not (the scalar branch)
    kinds = {(int(o) % 4 == 0, (mis - int(o)) % 4 == 0) for o, (n, mis) in zip(off['offset'], R.LAYOUTS['offset'])}
    assert {mis for _, mis in R.LAYOUTS['offset']} == {1, 2, 3}
    assert kinds == {(True, False), (False, False), (False, True)}
    lens = [n for n, _ in R.LAYOUTS['empty']]
    assert lens[0] == 0 and lens[-1] == 0 and any(a == b == 0 for a, b in zip(lens[1:-1], lens[2:-1]))
    # 'big': five workgroups of 256 threads x 4 elements take a second trip, the split is odd and inside it
    assert R.BIG_N == 8192 * 1024 + 5 * 1024 + 3 and R.BIG_SPLIT % 2 == 1 and 8192 * 1024 < R.BIG_SPLIT < R.BIG_N
    assert [n for n, _ in R.LAYOUTS['big']] == [R.BIG_SPLIT, R.BIG_N - R.BIG_SPLIT]
