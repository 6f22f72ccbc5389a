"""The fused angular-margin softmax head and ``batch_norm_rows`` (``csrc/aam_softmax.hip``) against a plain fp64 restatement of
``speaker_embeddings/loss.py:64-103`` (a boolean mask in place of the ``cat`` loop) and ``torch.nn.functional.batch_norm`` in fp64.

The gates are four times the largest error of the SAME restatement run in fp32 on the CPU against its fp64 run over these cases, relative
to the largest magnitude of the quantity in the case: ``profiles/aam_softmax_gates.txt`` (``scripts/aam_softmax_gates.py``) has the
measured figures, the gates and what the kernels achieved."""
import pytest
import torch
import torch.nn.functional as F

from padertorch_amd.ops.aam_softmax import DEFAULTS, kAamBM, kAamBN

pytestmark = pytest.mark.gpu

#: profiles/aam_softmax_gates.txt: 4 x the fp32 restatement's largest relative error per quantity
GATES = {'loss': 1.1e-6, 'de': 4.4e-6, 'dw': 4.2e-6, 'w_hat': 4.7e-7}
#: (dx: at B = 2 the batch-norm gradient is all cancellation - x_hat = +-1 - and the fp32 run of torch itself is off by 8e-4 of it)
BN_GATES = {'y': 4.1e-7, 'dx': 3.2e-3, 'running_mean': 3.7e-7, 'running_var': 3.6e-7}

#: (B, E, C, labels): one row and two classes (the label is the class farther from the embedding: with the nearer one the loss is
#: 1e-9, all cancellation, and measures nothing), the class tile's edge, a second batch tile with every label in the second class tile's only
#: class, three class tiles with the first class, the last class and duplicates
SHAPES = [(1, 6, 2, 'farthest'), (5, 6, kAamBN - 1, 'seeded'), (kAamBM + 5, 70, kAamBN + 1, 'last'), (37, 256, 2 * kAamBN + 3, 'edges')]


def inputs(B, E, C, labels, dtype=torch.float64):
    g = torch.Generator().manual_seed(B * 1000 + C)
    e = torch.randn(B, E, generator=g, dtype=torch.float64) * (10. ** torch.linspace(-1, 1, B))[:, None]     # row norms over 100 x
    w = torch.randn(C, E, generator=g, dtype=torch.float64)
    y = torch.randint(0, C, (B,), generator=g)
    if labels == 'farthest':
        y = (e @ w.T).argmin(1)
    elif labels == 'last':
        y[:] = C - 1
    elif labels == 'edges':
        y[:4] = torch.tensor([0, C - 1, 5, 5])
    gout = torch.randn(B, generator=g, dtype=torch.float64)
    return e.to(dtype), w.to(dtype), y, gout.to(dtype)


def restatement(e, w, y, loss_type, s, m, eps=1e-7, gout=None):
    """``(-L [B] or its mean, de, dW of the normalised rows, W_hat, cos_y)`` in the dtype of ``e``; ``gout=None``: ``reduce='mean'``."""
    e = e.clone().requires_grad_(True)
    w_hat = F.normalize(w, p=2, dim=1).requires_grad_(True)
    cos = F.normalize(e, p=2, dim=1) @ w_hat.T
    target = F.one_hot(y, w.shape[0]).bool()
    cos_y = cos[target]
    if loss_type == 'aam':
        n = s * (cos_y - m)
    elif loss_type == 'arcface':
        n = s * torch.cos(torch.acos(torch.clamp(cos_y, -1. + eps, 1 - eps)) + m)
    else:
        n = s * torch.cos(m * torch.acos(torch.clamp(cos_y, -1. + eps, 1 - eps)))
    L = n - torch.log(torch.exp(n) + torch.exp(s * cos).masked_fill(target, 0.).sum(1))
    loss = -L.mean() if gout is None else -L
    loss.backward(None if gout is None else gout)
    return loss.detach(), e.grad, w_hat.grad, w_hat.detach(), cos_y.detach()


def rel(got, want):
    return float((got.double().cpu() - want).abs().max() / want.abs().max())


def run(e, w, y, loss_type, reduce, gout, check=True):
    from padertorch_amd.ops.aam_softmax import angular_softmax_loss
    e = e.float().cuda().requires_grad_(True)
    w = w.float().cuda().requires_grad_(True)
    loss = angular_softmax_loss(e, w, y.cuda(), loss_type, reduce=reduce, check=check)
    loss.backward(None if reduce == 'mean' else gout.float().cuda())
    return loss.detach(), e.grad, w.grad, w.detach()


@pytest.mark.parametrize('reduce', ['mean', None])
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'x'.join(map(str, s)))
@pytest.mark.parametrize('loss_type', ['aam', 'arcface', 'sphereface'])
def test_loss_and_gradients_against_fp64(loss_type, shape, reduce):
    e, w, y, gout = inputs(*shape)
    want = restatement(e, w, y, loss_type, *DEFAULTS[loss_type], gout=None if reduce == 'mean' else gout)
    assert want[4].abs().max() <= 0.99                      # the clamp is never active: no gradient sits on its kink
    got = run(e, w, y, loss_type, reduce, gout)
    errors = {k: rel(a, b) for k, a, b in zip(GATES, got, want)}
    print(loss_type, shape, reduce, errors)
    for k in GATES:
        assert errors[k] <= GATES[k], (k, errors)


def test_range_clamp_active_and_opposite():
    """``cos_y = 1`` (clamp active) and ``cos_y = -1`` with arcface, s = 64: finite and equal to the fp64 restatement.  Tolerance: behind
    the clamp ``n = s cos(acos(c) + m)`` moves by at most ``s |acos(1 - eps) - acos(1 - eps - d)|`` for an error ``d`` of the fp32 cosine;
    ``d = E 2^-24`` (E = 8 products of unit vectors' elements) gives ``64 (1.08e-3 - 4.5e-4) = 0.04``, absolute."""
    C, E = kAamBN + 1, 8
    _, w, _, _ = inputs(2, E, C, 'seeded')
    y = torch.tensor([C - 1, 3])
    e = torch.stack([3. * w[C - 1], -0.5 * w[3]])
    want = restatement(e, w, y, 'arcface', 64., 0.5, gout=torch.ones(2, dtype=torch.float64))[0]
    got = run(e, w, y, 'arcface', None, torch.ones(2))[0]
    print(got, want)
    assert torch.isfinite(got).all()
    assert (got.double().cpu() - want).abs().max() <= 0.04


def test_label_out_of_range_is_nan_and_indexes_nothing():
    e, w, y, gout = inputs(5, 6, kAamBN - 1, 'seeded')
    bad = y.clone()
    bad[2] = kAamBN - 1                                     # == C
    loss, de, dw, _ = run(e, w, bad, 'aam', None, gout, check=False)
    keep = torch.tensor([0, 1, 3, 4])
    want = restatement(e[keep], w, y[keep], 'aam', *DEFAULTS['aam'], gout=gout[keep])
    assert torch.isnan(loss[2]) and rel(loss[keep], want[0]) <= GATES['loss']
    assert torch.isfinite(dw).all() and rel(dw, want[2]) <= GATES['dw']
    assert rel(de[keep], want[1]) <= GATES['de']


def test_capture_replays_other_labels_bit_identically():
    from padertorch_amd.ops.aam_softmax import angular_softmax_loss
    e, w, y, _ = inputs(37, 256, 2 * kAamBN + 3, 'edges')
    e, y2 = e.float().cuda(), y.flip(0).cuda()
    w = F.normalize(w.float().cuda(), dim=1)                # (normalising a normalised row again is not the identity bit for bit)

    def step(labels, e_, w_):
        loss = angular_softmax_loss(e_, w_, labels, 'arcface', check=False)
        return (loss, *torch.autograd.grad(loss, (e_, w_)))
    eager = [t.clone() for t in step(y2, e.clone().requires_grad_(True), w.clone().requires_grad_(True))]
    labels, es, ws = y.cuda().clone(), e.clone().requires_grad_(True), w.clone().requires_grad_(True)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step(labels, es, ws)                                # warm-up outside the capture
        with torch.no_grad():
            ws.copy_(w)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = step(labels, es, ws)
    for _ in range(3):                                      # several replays: each equal to the eager call on those labels
        labels.copy_(y2)
        with torch.no_grad():
            ws.copy_(w)
        graph.replay()
        torch.cuda.synchronize()
        for a, b in zip(out, eager):
            assert torch.equal(a, b)


@pytest.mark.parametrize('training', [True, False])
@pytest.mark.parametrize('B,E', [(2, 3), (37, 70)])
def test_batch_norm_rows_against_fp64(B, E, training):
    from padertorch_amd.ops.aam_softmax import batch_norm_rows
    g = torch.Generator().manual_seed(B)
    x = (torch.randn(B, E, generator=g, dtype=torch.float64) * 3 + 1).requires_grad_(True)
    gy = torch.randn(B, E, generator=g, dtype=torch.float64)
    rm, rv = torch.randn(E, generator=g, dtype=torch.float64), torch.rand(E, generator=g, dtype=torch.float64) + 0.5
    want_rm, want_rv = rm.clone(), rv.clone()
    F.batch_norm(x, want_rm, want_rv, training=training, momentum=0.1, eps=1e-5).backward(gy)
    xs = x.detach().float().cuda().requires_grad_(True)
    got_rm, got_rv, count = rm.float().cuda(), rv.float().cuda(), torch.tensor(4).cuda()
    ys = batch_norm_rows(xs, got_rm, got_rv, count, training, 0.1, 1e-5)
    ys.backward(gy.float().cuda())
    want_y = F.batch_norm(x.detach(), rm.clone(), rv.clone(), training=training, momentum=0.1, eps=1e-5)
    errors = {k: rel(a, b) for k, a, b in zip(BN_GATES, (ys.detach(), xs.grad, got_rm, got_rv), (want_y, x.grad, want_rm, want_rv))}
    print(B, E, training, errors)
    assert int(count) == 4 + int(training)
    for k in BN_GATES:
        assert errors[k] <= BN_GATES[k], (k, errors)
