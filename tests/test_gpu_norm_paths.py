"""Masked normalisation on the GPU (``csrc/norm.hip`` through ``modules.normalize`` / ``modules.Normalization``), forward AND backward,
against the fp64 oracle (``oracle/norm_np.py``) on every reduction path of ``ptmi_norm_reduce`` and both forms of
``ptmi_norm_elementwise``.  The cases and the proof that they reach those paths are in ``tests/test_norm_host.py``.

Error measure: max abs deviation over the max abs value of the fp64 result, over EVERY element.  Tolerance, per case and quantity:
8 times (``FACTOR`` of ``test_gpu_beamforming.py``) the deviation of the same oracle run in float32 from its float64 run - never
anything the kernels produce; a float32 deviation of exactly 0 asks for equality.  A case is computed once (oracle and kernels) and
shared by the tests that look at it.

Out of scope: the ``long long`` index instantiations (2^31 - 1 elements and more: an 8 GiB input) are not run.
"""
import functools

import numpy as np
import pytest
import torch

from oracle import norm_np as N
from test_gpu_beamforming import FACTOR, deviation
from test_norm_host import BY_NAME, EPS, NAMES, describe, make_inputs, oracle_args

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
QUANTITIES = ('y', 'mean', 'power', 'grad_x', 'grad_gamma', 'grad_beta')


def dev_tensor(a, view=None):
    """``a`` on the device; ``view='transposed'``: the same values as a non-contiguous view (last two axes swapped in memory)."""
    if a is None:
        return None
    if view == 'transposed':
        return torch.from_numpy(np.ascontiguousarray(np.swapaxes(a, -1, -2))).to(DEV).transpose(-1, -2)
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def host(t):
    return None if t is None else t.detach().cpu().numpy()


def oracle(c, i, dtype):
    y, mean, power, n = N.normalize(i['x'], i['gamma'], i['beta'], *oracle_args(c), dtype=dtype)
    gx, gg, gb = N.normalize_backward(i['w'], i['x'], i['gamma'], i['beta'], *oracle_args(c), dtype=dtype)
    out = dict(y=y, mean=mean, power=power, n_values=n, grad_x=gx, grad_gamma=gg, grad_beta=gb)
    assert all(v is None or v.dtype == dtype for v in out.values())
    return out


def run_kernels(c, i):
    """One forward and backward of ``modules.normalize``: every output and gradient as numpy, bits as the device left them."""
    from padertorch_amd.modules import normalize
    x = dev_tensor(i['x'], c['view']).requires_grad_()
    assert x.is_contiguous() == (c['view'] is None)
    gamma, beta = (None if i[k] is None else dev_tensor(i[k]).requires_grad_() for k in ('gamma', 'beta'))
    y, mean, power, n = normalize(x, gamma, beta, *oracle_args(c))
    if c['loss'] == 'sum':
        y.sum().backward()                          # grad_y arrives as an expanded scalar
    else:
        (y * dev_tensor(i['w'])).sum().backward()
    torch.cuda.synchronize()
    return dict(y=host(y), mean=host(mean), power=host(power), n_values=host(n), grad_x=host(x.grad),
                grad_gamma=None if gamma is None else host(gamma.grad), grad_beta=None if beta is None else host(beta.grad))


def tolerances(single, want):
    return {k: FACTOR * deviation(single[k], want[k]) for k in want if want[k] is not None}


def report(title, got, want, tol, keys):
    """Print error and tolerance per quantity; return the quantities that miss (all are printed before any assertion)."""
    errors = {k: deviation(got[k], want[k]) for k in keys if want[k] is not None}
    print(f'\n{title}\n    ' + ', '.join(f'{k} {e:.2e} (tol {tol[k]:.2e})' for k, e in errors.items()))
    return {k: (e, tol[k]) for k, e in errors.items() if not e <= tol[k]}


@functools.lru_cache(maxsize=None)
def case(name):
    """Inputs, the fp64 oracle, the tolerances from its float32 run and the kernels' results: once per case."""
    c = BY_NAME[name]
    i = make_inputs(c)
    want = oracle(c, i, np.float64)
    return dict(c=c, inputs=i, want=want, tol=tolerances(oracle(c, i, np.float32), want), got=run_kernels(c, i))


def valid(c):
    return N.compute_mask(c['shape'], c['lens'], c['batch_axis'], c['sequence_axis']) > 0


@pytest.mark.parametrize('name', NAMES)
def test_outputs_and_gradients_against_the_fp64_oracle(name):
    k = case(name)
    c, got, want = k['c'], k['got'], k['want']
    for q in QUANTITIES + ('n_values',):
        assert (got[q] is None) == (want[q] is None), q
        assert got[q] is None or (got[q].shape == want[q].shape and got[q].dtype == np.float32), q
    missed = report(f'{name} {c["shape"]}: {describe(c)}', got, want, k['tol'], QUANTITIES)
    assert np.array_equal(got['n_values'], want['n_values'])
    assert not missed, missed


@pytest.mark.parametrize('name', [n for n in NAMES if BY_NAME[n]['lens'] is not None])
def test_masked_positions_are_exactly_zero(name):
    k = case(name)
    tail = ~valid(k['c'])
    assert tail.any()
    assert not k['got']['y'][tail].any() and not k['got']['grad_x'][tail].any()
    empty = k['want']['n_values'] == 0              # a length of 0: n = 0, mean = power = 0
    assert not k['got']['mean'][empty].any() and not k['got']['power'][empty].any()


@pytest.mark.parametrize('name', NAMES)
def test_a_second_run_gives_the_same_bits(name):
    k = case(name)
    again = run_kernels(k['c'], k['inputs'])
    for q, v in k['got'].items():
        assert v is None or np.array_equal(again[q], v), q


@pytest.mark.parametrize('name', [n for n in NAMES if BY_NAME[n]['lens'] is not None])
def test_nan_behind_the_lengths_changes_no_bit(name):
    k = case(name)
    tail = ~valid(k['c'])
    i = dict(k['inputs'])
    i['x'], i['w'] = i['x'].copy(), i['w'].copy()
    i['x'][tail] = np.nan
    if k['c']['loss'] != 'sum':
        i['w'][tail] = np.nan
    changed = run_kernels(k['c'], i)
    for q, v in k['got'].items():
        assert v is None or np.array_equal(changed[q], v), q


# ---- running statistics through the module: two training steps, one evaluation step (the fixed-statistics path) --------------------------
def _module_oracle(c, steps, ev, gamma, beta, momentum, dtype):
    """Buffers after every training step, then ``y`` and the gradients of the evaluation step, all in ``dtype``."""
    state = dict(num_tracked_values=np.zeros((1, 5, 1)), running_mean=np.zeros((1, 5, 1)), running_power=np.ones((1, 5, 1)))
    out = {}
    for s, i in enumerate(steps):
        _, mean, power, n = N.normalize(i['x'], gamma, beta, *oracle_args(c), dtype=dtype)
        state = N.update_running_stats(state, mean, power, n, momentum, dtype=dtype)
        out.update({f'step {s} {b}': v for b, v in state.items()})
    args = (state, gamma, beta, c['batch_axis'], c['sequence_axis'], c['lens'], True, True, EPS)
    out['y'] = N.running_norm(ev['x'], *args, dtype=dtype)
    out['grad_x'], out['grad_gamma'], out['grad_beta'] = N.running_norm_backward(ev['w'], ev['x'], *args, dtype=dtype)
    assert all(v.dtype == dtype for v in out.values())
    return out


def test_module_tracks_running_statistics_and_evaluates_with_them():
    from padertorch_amd.modules import Normalization
    c = BY_NAME['bct bt-c']
    steps, ev = [make_inputs(c, seed=1), make_inputs(c, seed=2)], make_inputs(c, seed=3)
    gamma, beta = steps[0]['gamma'], steps[0]['beta']
    m = Normalization('bct', (None, 5, None), statistics_axis='bt').to(DEV)
    assert m.track_running_stats and m.eps == EPS
    with torch.no_grad():
        m.gamma.copy_(dev_tensor(gamma))
        m.beta.copy_(dev_tensor(beta))
    want = _module_oracle(c, steps, ev, gamma, beta, m.momentum, np.float64)
    tol = tolerances(_module_oracle(c, steps, ev, gamma, beta, m.momentum, np.float32), want)
    got = {}
    m.train()
    for s, i in enumerate(steps):
        m(dev_tensor(i['x']), c['lens'])
        got.update({f'step {s} {b}': host(getattr(m, b)) for b in ('num_tracked_values', 'running_mean', 'running_power')})
    m.eval()
    x = dev_tensor(ev['x']).requires_grad_()
    y = m(x, c['lens'])
    (y * dev_tensor(ev['w'])).sum().backward()
    got.update(y=host(y), grad_x=host(x.grad), grad_gamma=host(m.gamma.grad), grad_beta=host(m.beta.grad))
    missed = report('Normalization(bct, bt) (4, 5, 600): two training steps, one evaluation step', got, want, tol, list(want))
    for s in range(2):
        assert np.array_equal(got[f'step {s} num_tracked_values'], want[f'step {s} num_tracked_values'])
    assert not missed, missed
    tail = ~valid(c)
    assert not got['y'][tail].any() and not got['grad_x'][tail].any()
