"""``gaussian_kl_divergence`` (``csrc/gauss_kl.hip``) against a plain fp64 restatement of ``padertorch/ops/losses/kl_divergence.py:17-60``
with torch autograd on the CPU (``solve_triangular`` on ``T.tril()`` in place of the general inverse).

The gates are four times the largest error of the explicit formulas of DESIGN.md 3.5v evaluated in fp32 on the CPU against that fp64
restatement over these cases, relative to the largest magnitude of the quantity in the case (``scripts/gauss_kl_gates.py``,
``profiles/gauss_kl_gates.txt``)."""
import pytest
import torch
from torch.distributions import MultivariateNormal, Normal

from padertorch_amd.ops.losses.kl_divergence import kGklSplitRows

pytestmark = pytest.mark.gpu

#: profiles/gauss_kl_gates.txt: 4 x the fp32 formulas' largest relative error per quantity and prior kind
GATES = {True: {'kl': 8.2e-7, 'dmu': 9.0e-7, 'dsigma': 6.8e-7, 'dm': 1.6e-6, 'dscale': 1.8e-6},
         False: {'kl': 1.0e-6, 'dmu': 8.3e-7, 'dsigma': 6.7e-7, 'dm': 1.3e-6, 'dscale': 2.5e-6}}

#: (B, K, D): the smallest | D no multiple of 4 | across the 64-row tile and 16 components, D one MFMA tile | D across 32 | the largest D,
#: two row tiles and a remainder | more than two row splits of the component-owning kernel
SHAPES = [(1, 1, 1), (19, 3, 5), (70, 17, 16), (33, 5, 37), (130, 2, 64), (2 * kGklSplitRows + 3, 3, 20)]
CASES = [(*s, full) for full in (True, False) for s in SHAPES]


def inputs(B, K, D, full, dtype=torch.float64):
    """``(mu, sigma [B, D], m [K, D], scale_tril [K, D, D] or scale [K, D], G [B, K])``."""
    g = torch.Generator().manual_seed(1000 * B + 10 * K + full)

    def randn(*shape):
        return torch.randn(*shape, generator=g, dtype=torch.float64)

    def rand(*shape):
        return torch.rand(*shape, generator=g, dtype=torch.float64)
    mu, m, sigma = randn(B, D), randn(K, D), 0.2 + rand(B, D)
    if full:
        scale = torch.diag_embed(0.5 + rand(K, D)) + 0.5 * torch.tril(randn(K, D, D), -1) / D ** 0.5
    else:
        scale = 0.5 + rand(K, D)
    return [x.to(dtype) for x in (mu, sigma, m, scale, randn(B, K))]


def restatement(mu, sigma, m, scale, G):
    """``(kl, dmu, dsigma, dm, dscale)`` in the dtype of ``mu``; ``scale.dim() == 3``: the full-covariance prior."""
    mu, sigma, m, scale = (x.clone().requires_grad_(True) for x in (mu, sigma, m, scale))
    D = mu.shape[1]
    diff = m[None] - mu[:, None]
    if scale.dim() == 3:
        T = scale.tril()
        L = torch.linalg.solve_triangular(T, torch.eye(D, dtype=mu.dtype).expand_as(T), upper=False)
        y = torch.linalg.solve_triangular(T, diff.permute(1, 2, 0), upper=False)
        kl = torch.diagonal(T, dim1=1, dim2=2).log().sum(-1)[None] - sigma.log().sum(-1)[:, None] + \
            0.5 * (sigma.pow(2) @ L.pow(2).sum(-2).T + y.pow(2).sum(1).T - D)
    else:
        kl = (scale.log()[None] - sigma.log()[:, None] + (sigma.pow(2)[:, None] + diff.pow(2)) / (2 * scale.pow(2))[None] - 0.5).sum(-1)
    return (kl.detach(), *torch.autograd.grad((kl * G).sum(), (mu, sigma, m, scale)))


def run(mu, sigma, m, scale, G):
    from padertorch_amd.ops import gaussian_kl_divergence
    mu, sigma, m, scale = (x.float().cuda().requires_grad_(True) for x in (mu, sigma, m, scale))
    p = MultivariateNormal(m, scale_tril=scale, validate_args=False) if scale.dim() == 3 else Normal(m, scale)
    kl = gaussian_kl_divergence(Normal(mu, sigma), p)
    return (kl.detach(), *torch.autograd.grad((kl * G.float().cuda()).sum(), (mu, sigma, m, scale)))


@pytest.mark.parametrize('case', CASES, ids=lambda c: '-'.join(str(v) for v in c))
def test_against_fp64(case):
    B, K, D, full = case
    data = inputs(B, K, D, full)
    want, got = restatement(*data), run(*data)
    if full and D > 1:
        assert not got[4].triu(1).any()                     # scale_tril's upper triangle gets no gradient
        want = (*want[:4], want[4].tril())
    errors = {k: float((a.double().cpu() - w).abs().max() / w.abs().max()) for k, a, w in zip(GATES[full], got, want)}
    print(case, errors)
    for k, gate in GATES[full].items():
        assert errors[k] <= gate, (k, errors)


@pytest.mark.parametrize('full', [True, False])
def test_batch_shapes_and_strides(full):
    from padertorch_amd.ops import gaussian_kl_divergence
    mu, _, m, scale, _ = (x.float().cuda() for x in inputs(20, 6, 7, full))
    sigma = (0.2 + torch.rand(4, 7, device='cuda'))[:, None].expand(4, 5, 7)
    assert not sigma.is_contiguous()
    if full:
        p, flat = (MultivariateNormal(m.view(*s, 7), scale_tril=scale.view(*s, 7, 7), validate_args=False) for s in ((3, 2), (6,)))
    else:
        p, flat = (Normal(m.view(*s, 7), scale.view(*s, 7)) for s in ((3, 2), (6,)))
    kl = gaussian_kl_divergence(Normal(mu.view(4, 5, 7), sigma), p)
    assert kl.shape == (4, 5, 3, 2)
    assert torch.equal(kl.reshape(20, 6), gaussian_kl_divergence(Normal(mu, sigma.reshape(20, 7).contiguous()), flat))


@pytest.mark.parametrize('full', [True, False])
def test_capture_replays_other_inputs_bit_identically(full):
    from padertorch_amd.ops import gaussian_kl_divergence
    *params, G = (x.float().cuda() for x in inputs(*SHAPES[2], full))
    other = [x.float().cuda() for x in inputs(*SHAPES[2], not full)[:3]] + [params[3].flip(0).contiguous()]

    def step(mu, sigma, m, scale):
        p = MultivariateNormal(m, scale_tril=scale, validate_args=False) if full else Normal(m, scale, validate_args=False)
        kl = gaussian_kl_divergence(Normal(mu, sigma, validate_args=False), p)
        return (kl, *torch.autograd.grad((kl * G).sum(), (mu, sigma, m, scale)))
    eager = [x.detach().clone() for x in step(*[x.clone().requires_grad_(True) for x in other])]
    held = [x.clone().requires_grad_(True) for x in params]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step(*held)                                         # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = step(*held)
    for _ in range(3):                                      # several replays: each equal to the eager call on those inputs
        with torch.no_grad():
            for h, o in zip(held, other):
                h.copy_(o)
        graph.replay()
        torch.cuda.synchronize()
        for a, c in zip(out, eager):
            assert torch.equal(a.detach(), c)
