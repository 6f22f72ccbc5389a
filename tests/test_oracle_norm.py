"""Oracle masked normalisation (oracle/norm_np.py) vs the reference goldens g9 (CPU)."""
import numpy as np
import pytest

from oracle import norm_np as N
from test_norm_host import BY_NAME, NAMES, make_inputs, oracle_args


def test_normalize_vs_reference(g9):
    for c in g9['cases']:
        k = c['key']
        y, mean, power, n = N.normalize(g9[f'{k}/x'], g9.get(f'{k}/gamma'), g9.get(f'{k}/beta'), c['axes'], c['b_ax'],
                                        c['t_ax'], c['lens'], c['shift'], c['scale'], 1e-3)
        np.testing.assert_allclose(y, g9[f'{k}/y'], rtol=2e-5, atol=2e-5)
        np.testing.assert_allclose(mean, g9[f'{k}/mean'], rtol=1e-5, atol=1e-6)
        np.testing.assert_allclose(power, g9[f'{k}/power'], rtol=1e-5, atol=1e-6)
        np.testing.assert_array_equal(n, g9[f'{k}/n'])            # counts: exact


def test_doctest_statistics():
    """normalization.py:424-466: x = 2, lengths [1, 2, 3] -> mean 2, power 4, n 6."""
    y, m, p, n = N.normalize(2 * np.ones((3, 10, 4)), None, None, [0, 2], 0, 2, [1, 2, 3], True, True, 1e-3)
    assert (m == 2).all() and (p == 4).all() and (n == 6).all() and m.shape == (1, 10, 1)
    assert (y == 0).all()


def test_running_statistics_and_eval(g9):
    for mod in g9['modules']:
        k = mod['key']
        gamma, beta = g9[f'{k}/gamma'], g9[f'{k}/beta']
        state = dict(num_tracked_values=np.zeros((1, 4, 1)), running_mean=np.zeros((1, 4, 1)),
                     running_power=np.ones((1, 4, 1)))
        for step in range(3):
            x, lens = g9[f'{k}/s{step}/x'], g9[f'{k}/s{step}/lens'].tolist()
            y, mean, power, n = N.normalize(x, gamma, beta, [0, 2], 0, 2, lens, True, True, 1e-5)
            state = N.update_running_stats(state, mean, power, n, mod['momentum'])
            if mod['cls'] == 'inorm':      # InputNormalization: update first, then normalise with the running stats
                y = N.running_norm(x, state, gamma, beta, 0, 2, lens, True, True, 1e-5)
            np.testing.assert_allclose(y, g9[f'{k}/s{step}/y'], rtol=1e-4, atol=1e-4)
            for b in ('num_tracked_values', 'running_mean', 'running_power'):
                np.testing.assert_allclose(state[b], g9[f'{k}/s{step}/{b}'], rtol=1e-5, atol=1e-6)
        y = N.running_norm(g9[f'{k}/eval/x'], state, gamma, beta, 0, 2, [5, 2], True, True, 1e-5)
        np.testing.assert_allclose(y, g9[f'{k}/eval/y'], rtol=1e-4, atol=1e-4)


def _torch_forward(x, gamma, beta, axes, b_ax, t_ax, lens, shift, scale, eps):
    """The forward of ``normalization.py:414-494`` in torch ops, for autograd: masked statistics, clamp, affine, mask."""
    import torch
    mask = torch.ones_like(x)
    if lens is not None:
        sb, st = [1] * x.dim(), [1] * x.dim()
        sb[b_ax], st[t_ax] = -1, -1
        mask = (torch.arange(x.shape[t_ax]).reshape(st) < torch.tensor(lens).reshape(sb)).to(x.dtype).expand_as(x)
    den = mask.sum(dim=axes, keepdim=True).clamp(min=1)
    xm = x * mask
    mean = xm.sum(dim=axes, keepdim=True) / den
    power = (xm ** 2).sum(dim=axes, keepdim=True) / den
    y = xm - mean if shift else xm
    if scale:
        y = y / torch.sqrt((power - mean ** 2 if shift else power).clamp(min=0) + eps)
    if gamma is not None:
        y = y * gamma
    if beta is not None:
        y = y + beta
    return y * mask, mean, power


@pytest.mark.parametrize('name', NAMES)
def test_backward_oracle_vs_float64_autograd(name):
    """``normalize_backward`` against torch's float64 autograd of the forward above, on every case of the GPU tests' table.  Both sides
    are float64 sums of at most 10^4 terms: each within ``n u ~ 1e-12`` of the exact value relative to the terms' size; 1e-10 leaves
    room for the cancellation between the three terms of ``grad_x`` and is far below any error of the formula."""
    import torch
    c = BY_NAME[name]
    i = make_inputs(c)
    t = {k: None if v is None else torch.tensor(v, dtype=torch.float64, requires_grad=k != 'w') for k, v in i.items()}
    y, mean, power = _torch_forward(t['x'], t['gamma'], t['beta'], *oracle_args(c))
    (y * t['w']).sum().backward()
    want = dict(y=y, mean=mean, power=power, grad_x=t['x'].grad, grad_gamma=None if t['gamma'] is None else t['gamma'].grad,
                grad_beta=None if t['beta'] is None else t['beta'].grad)
    y, mean, power, _ = N.normalize(i['x'], i['gamma'], i['beta'], *oracle_args(c))
    gx, gg, gb = N.normalize_backward(i['w'], i['x'], i['gamma'], i['beta'], *oracle_args(c))
    got = dict(y=y, mean=mean, power=power, grad_x=gx, grad_gamma=gg, grad_beta=gb)
    for k, w in want.items():
        assert (got[k] is None) == (w is None), k
        if w is not None:
            w = w.detach().numpy()
            assert got[k].shape == w.shape and got[k].dtype == np.float64, k
            assert np.abs(got[k] - w).max() <= 1e-10 * np.abs(w).max(), (k, np.abs(got[k] - w).max() / np.abs(w).max())


def test_backward_oracle_vs_reference_gradients(g9):
    """The goldens' gradients (the reference's hand-written backward) at the tolerances ``test_gpu_norm.py`` holds the kernels to."""
    for c in g9['cases']:
        k = c['key']
        gx, gg, gb = N.normalize_backward(g9[f'{k}/w'], g9[f'{k}/x'], g9.get(f'{k}/gamma'), g9.get(f'{k}/beta'), c['axes'], c['b_ax'],
                                          c['t_ax'], c['lens'], c['shift'], c['scale'], 1e-3)
        np.testing.assert_allclose(gx, g9[f'{k}/grad_x'], rtol=2e-4, atol=2e-5, err_msg=k)
        for got, name in ((gg, 'grad_gamma'), (gb, 'grad_beta')):
            assert (got is None) == (f'{k}/{name}' not in g9), (k, name)
            if got is not None:
                np.testing.assert_allclose(got, g9[f'{k}/{name}'], rtol=2e-4, atol=2e-5, err_msg=k)


def test_float32_run_of_the_oracle_stays_float32():
    """The GPU tests' tolerances are the float32 run's deviation from the float64 run: nothing in it may be promoted."""
    c = BY_NAME['bct bt-c']
    i = make_inputs(c)
    out = N.normalize(i['x'], i['gamma'], i['beta'], *oracle_args(c), dtype=np.float32)
    out += N.normalize_backward(i['w'], i['x'], i['gamma'], i['beta'], *oracle_args(c), dtype=np.float32)
    state = dict(num_tracked_values=np.zeros((1, 5, 1)), running_mean=np.zeros((1, 5, 1)), running_power=np.ones((1, 5, 1)))
    state = N.update_running_stats(state, *out[1:4], 0.95, dtype=np.float32)
    args = (state, i['gamma'], i['beta'], c['batch_axis'], c['sequence_axis'], c['lens'], True, True, 1e-5)
    out += tuple(state.values()) + (N.running_norm(i['x'], *args, dtype=np.float32),)
    out += N.running_norm_backward(i['w'], i['x'], *args, dtype=np.float32)
    assert all(a.dtype == np.float32 for a in out), [a.dtype for a in out]


def test_running_norm_backward_vs_float64_autograd():
    import torch
    c = BY_NAME['bct bt-c']
    i = make_inputs(c)
    rng = np.random.default_rng(3)
    state = dict(num_tracked_values=np.full((1, 5, 1), 1300.), running_mean=rng.standard_normal((1, 5, 1)),
                 running_power=2 + rng.uniform(size=(1, 5, 1)))
    t = {k: torch.tensor(v, dtype=torch.float64, requires_grad=k != 'w') for k, v in i.items()}
    s = {k: torch.tensor(v) for k, v in state.items()}
    n = s['num_tracked_values'].clamp(min=2)
    var = (n / (n - 1) * s['running_power'] - s['running_mean'] ** 2).clamp(min=0) + 1e-5
    mask = (torch.arange(600)[None, None] < torch.tensor(c['lens'])[:, None, None]).double()
    y = ((t['x'] - s['running_mean']) / torch.sqrt(var + 1e-5) * t['gamma'] + t['beta']) * mask
    (y * t['w']).sum().backward()
    args = (state, i['gamma'], i['beta'], c['batch_axis'], c['sequence_axis'], c['lens'], True, True, 1e-5)
    got = (N.running_norm(i['x'], *args),) + N.running_norm_backward(i['w'], i['x'], *args)
    for g, w in zip(got, (y, t['x'].grad, t['gamma'].grad, t['beta'].grad)):
        w = w.detach().numpy()
        assert g.shape == w.shape and np.abs(g - w).max() <= 1e-10 * np.abs(w).max()


def test_unit_norm_oracle_matches_torch_normalize():
    """oracle.norm_np.unit_norm / unit_norm_backward == torch.nn.functional.normalize(dim=-2) and its
    autograd (the op of padertorch/contrib/tcl/dc.py:70), incl. all-zero vectors (eps clamp)."""
    import torch
    from oracle import norm_np
    rng = np.random.default_rng(5)
    for shape in [(7, 20, 257), (3, 4, 9), (1, 1, 1), (5, 32, 12)]:
        x = rng.standard_normal(shape).astype(np.float32)
        x[0, :, 0] = 0.0                                   # clamped norm
        g = rng.standard_normal(shape).astype(np.float32)
        xt = torch.tensor(x, requires_grad=True)
        yt = torch.nn.functional.normalize(xt, dim=-2)
        (yt * torch.tensor(g)).sum().backward()
        np.testing.assert_allclose(norm_np.unit_norm(x), yt.detach().numpy(), rtol=1e-6, atol=1e-7)
        np.testing.assert_allclose(norm_np.unit_norm_backward(g, x), xt.grad.numpy(), rtol=2e-5, atol=1e-6)
