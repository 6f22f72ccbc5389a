"""A second backward pass through the same graph, for every HIP ``autograd.Function`` of ``padertorch_amd.ops``.

``torch.nn.LSTM`` and the reference's plain modules support ``backward(retain_graph=True)`` twice and ``torch.autograd.grad`` called
twice on one graph; an op whose forward leaves device state for ONE backward to consume (the BLSTM's forward recurrence prefills its
backward scratch: data-as-flag pattern, zeroed bias sums, arrival and error words) must not hand a second pass the first one's
leftovers.  Per op, at small sizes, against an fp64 reference of the same operation (``torch.nn.LSTM`` / ``Linear`` / the oracle's
losses) at the tolerances of the op's own tests:

  (a) ``backward(g, retain_graph=True)`` twice accumulates exactly twice the reference gradient;
  (b) ``torch.autograd.grad`` with cotangent g1 (``retain_graph=True``), then with g2 != g1, gives each call the reference gradient of
      its own cotangent.

The LSTM runs on the uniform, ragged-packed and ``StaticSlots`` routes, at H = 600 (persistent split kernels) and a small H, with one
and two directions, and with in-place weight gradients (``OpContext(defer_wgrad=True)``: the route whose backward recurrence hands the
gate gradients on as planes).
"""
import pytest
import torch
from torch.nn.utils.rnn import PackedSequence, pack_sequence, pad_packed_sequence

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def _close(got, want, atol, rtol=0., what=''):
    got, want = got.detach().cpu().double(), want.detach().cpu().double()
    assert got.shape == want.shape, (what, got.shape, want.shape)
    err = (got - want).abs() - rtol * want.abs()
    assert float(err.max()) <= atol, (what, float((got - want).abs().max()), atol)


def _twice(f, inputs, ref, cotangents, tol):
    """(a) and (b) for ``out = f(*inputs)`` against ``ref(*inputs_in_fp64)``; ``tol(reference gradient) -> (atol, rtol)``."""
    x64 = [x.detach().cpu().double().requires_grad_(True) for x in inputs]
    out64 = ref(*x64)
    want = []
    for g in cotangents:
        want.append(torch.autograd.grad(out64, x64, g.detach().cpu().double(), retain_graph=True))
    for x in inputs:
        x.grad = None
    out = f(*inputs)
    out.backward(cotangents[0], retain_graph=True)
    out.backward(cotangents[0], retain_graph=True)
    for i, (x, w) in enumerate(zip(inputs, want[0])):
        _close(x.grad, 2 * w, *tol(2 * w), what=('backward twice', i))
    for g, w in zip(cotangents, want):
        got = torch.autograd.grad(out, inputs, g, retain_graph=True)
        for i, (a, b) in enumerate(zip(got, w)):
            _close(a, b, *tol(b), what=('autograd.grad', i))


def _rel(k):
    return lambda w: (k * max(float(w.abs().max()), 1e-30), 0.)


# ------------------------------------------------------------------------------------------------------------------------- LSTM
LSTM_ROUTES = {
    # name: (frames per example, StaticSlots (slots, spare steps) or None)
    'uniform': ([12] * 16, None),
    'ragged': ([13, 11, 11, 8, 5, 2, 1], None),
    'slots': ([13, 11, 9, 8, 5, 4, 2, 1], (4, 3)),
    'slots16': ([13, 12, 11, 11, 10, 9, 8, 8, 7, 6, 6, 5, 4, 3, 2, 2, 1, 1, 1, 1], (16, 2)),
}


def _lstm_forward(lstm, route):
    """padded input ``[B, T, I]`` -> padded output ``[B, T, ndir H]`` through ``ops.packed_lstm`` on the route's layout."""
    from padertorch_amd.ops import packed_lstm
    from padertorch_amd.ops.sequence import SlotLayout, StaticSlots
    lens, slots = LSTM_ROUTES[route]
    B, T = len(lens), max(lens)
    if slots is None:
        def f(xp):
            y = packed_lstm(lstm, pack_sequence([xp[b, :n] for b, n in enumerate(lens)]))
            return pad_packed_sequence(y, batch_first=True, total_length=T)[0]
        return f
    S, spare = slots
    st = StaticSlots(B, S, SlotLayout(lens, S).T + spare, T, DEV).set(lens)

    def f(xp):
        x = st.scatter_rows(xp)
        y = packed_lstm(lstm, PackedSequence(x, torch.full((st.steps,), S, dtype=torch.int64)), meta=st.meta).data
        return st.gather_rows(y)
    return f


def _lstm_reference(ref, lens):
    def f(xp):
        y, _ = ref(pack_sequence([xp[b, :n] for b, n in enumerate(lens)]))
        return pad_packed_sequence(y, batch_first=True, total_length=max(lens))[0]
    return f


@pytest.mark.parametrize('route,H,ndir,defer', [
    (r, H, d, False) for r in ('uniform', 'ragged', 'slots') for H in (600, 24) for d in (1, 2)] + [
    ('uniform', 600, 2, True), ('slots16', 600, 2, True), ('slots', 24, 2, True)])
def test_lstm_second_backward(route, H, ndir, defer, monkeypatch):
    """The BLSTM's backward scratch serves one pass; a second one - (a) and (b) - fills its own: every gradient (input, both weights,
    bias) against ``torch.nn.LSTM`` in fp64.  With ``defer``: weight gradients accumulated in place into ``.grad`` (the Trainer's
    route), (b) then asks autograd for the input gradient and ``.grad`` holds the weight gradients of g1 + g2."""
    from padertorch_amd.ops import lstm as L
    from padertorch_amd.ops import context as _context
    monkeypatch.setattr(L, 'CHECK_PERSISTENT_ERRORS', True)
    lens = LSTM_ROUTES[route][0]
    B, T, I = len(lens), max(lens), 20
    torch.manual_seed(H + ndir + B)
    ref = torch.nn.LSTM(I, H, 2, bidirectional=ndir == 2).double()
    lstm = torch.nn.LSTM(I, H, 2, bidirectional=ndir == 2)
    lstm.load_state_dict({k: v.float() for k, v in ref.state_dict().items()})
    lstm = lstm.to(DEV)
    params = list(lstm.parameters())
    if defer:
        for p in params:
            p.grad = torch.zeros_like(p)
        _context.attach(lstm, _context.OpContext(defer_wgrad=True))
        L.warm_side_stream(torch.device(DEV))
    mask = torch.zeros(B, T, 1)
    for b, n in enumerate(lens):
        mask[b, :n] = 1.
    xp = (torch.randn(B, T, I) * mask).to(DEV).requires_grad_(True)
    gs = [(torch.randn(B, T, ndir * H) * mask).to(DEV) for _ in range(2)]
    f, f64 = _lstm_forward(lstm, route), _lstm_reference(ref, lens)
    # tolerances of tests/test_gpu_lstm.py: the packed path against torch.nn.LSTM, and the in-place / H = 600 path
    tx = (2e-4, 0.) if (defer or H == 600) else (2e-5, 1e-4)
    tp = 3e-4 if (defer or H == 600) else 3e-5

    def want(g):
        x64 = xp.detach().cpu().double().requires_grad_(True)
        return torch.autograd.grad(f64(x64), [x64] + list(ref.parameters()), g.cpu().double())

    def check(got, w, what):
        sx = max(1., float(w[0].abs().max()))
        _close(got[0], w[0], tx[0] * sx, tx[1], what=(what, 'input'))
        for (name, _), a, b in zip(lstm.named_parameters(), got[1:], w[1:]):
            _close(a, b, tp * max(1., float(b.abs().max())), what=(what, name))

    def settle():
        L.sync_deferred()
        torch.cuda.synchronize()
        L.check_errors()
    w1, w2 = want(gs[0]), want(gs[1])
    # which scratch each layer's backward pass starts from: the forward's prefilled one (2) for the first pass only
    prefilled = []
    plain = L._LstmLayerFn.backward

    def spy(ctx, *grads):
        prefilled.append(int(ctx.scratch_b[1]))
        return plain(ctx, *grads)
    monkeypatch.setattr(L._LstmLayerFn, 'backward', staticmethod(spy))
    # (a) backward twice: twice the gradient of one
    out = f(xp)
    out.backward(gs[0], retain_graph=True)
    assert prefilled == [2, 2], prefilled              # (both layers: the route a stale second pass would take)
    out.backward(gs[0], retain_graph=True)
    assert prefilled == [2, 2, 0, 0], prefilled
    settle()
    check([xp.grad] + [p.grad for p in params], [2 * v for v in w1], 'backward twice')
    # (b) autograd.grad with g1, then g2, on one graph
    out = f(xp)
    if defer:
        for p in params:
            p.grad.zero_()
        got = [torch.autograd.grad(out, [xp], g, retain_graph=True)[0] for g in gs]
        settle()
        for g, w, what in zip(got, (w1, w2), ('grad g1', 'grad g2')):
            _close(g, w[0], tx[0] * max(1., float(w[0].abs().max())), tx[1], what=(what, 'input'))
        for (name, p), a, b in zip(lstm.named_parameters(), w1[1:], w2[1:]):
            _close(p.grad, a + b, tp * max(1., float((a + b).abs().max())), what=('.grad after grad g1, g2', name))
    else:
        for g, w, what in zip(gs, (w1, w2), ('grad g1', 'grad g2')):
            got = torch.autograd.grad(out, [xp] + params, g, retain_graph=True)
            settle()
            check(got, w, what)


# ---------------------------------------------------------------------------------------------------------------- dense layers
@pytest.mark.parametrize('relu', [False, True])
def test_linear_second_backward(relu):
    """``ops.linear`` (split-fp16 planes GEMM; ``relu``: the ReLU in the GEMM's epilogue) against ``torch.nn.Linear`` in fp64."""
    from padertorch_amd.ops.linear import linear
    torch.manual_seed(11 + relu)
    mod = torch.nn.Linear(48, 40).to(DEV)
    x = torch.randn(37, 48, device=DEV, requires_grad=True)
    w, b = mod.weight, mod.bias

    def ref(x, w, b):
        y = torch.nn.functional.linear(x, w, b)
        return torch.relu(y) if relu else y
    gs = [torch.randn(37, 40, device=DEV) for _ in range(2)]
    _twice(lambda x, w, b: linear(mod, x, activation='relu' if relu else None), [x, w, b], ref, gs, _rel(1e-5))


def test_linear_deferred_weight_gradient_second_backward():
    """``ops.linear`` with ``OpContext(defer_wgrad=True)``: the weight gradient is accumulated in place into ``.grad`` (side stream) -
    twice for two passes, g1 + g2 for two ``autograd.grad`` calls; the input gradient comes back as usual."""
    from padertorch_amd.ops import context as _context
    from padertorch_amd.ops import lstm as L
    from padertorch_amd.ops.linear import linear
    torch.manual_seed(12)
    mod = torch.nn.Linear(48, 40).to(DEV)
    mod.weight.grad, mod.bias.grad = torch.zeros_like(mod.weight), torch.zeros_like(mod.bias)
    _context.attach(mod, _context.OpContext(defer_wgrad=True))
    L.warm_side_stream(torch.device(DEV))
    x = torch.randn(37, 48, device=DEV, requires_grad=True)
    gs = [torch.randn(37, 40, device=DEV) for _ in range(2)]
    x64, w64, b64 = (t.detach().cpu().double().requires_grad_(True) for t in (x, mod.weight, mod.bias))
    y64 = torch.relu(torch.nn.functional.linear(x64, w64, b64))
    want = [torch.autograd.grad(y64, [x64, w64, b64], g.cpu().double(), retain_graph=True) for g in gs]
    y = linear(mod, x, activation='relu')
    y.backward(gs[0], retain_graph=True)
    y.backward(gs[0], retain_graph=True)
    L.sync_deferred()
    torch.cuda.synchronize()
    for got, w in zip((x.grad, mod.weight.grad, mod.bias.grad), want[0]):
        _close(got, 2 * w, 1e-5 * float(w.abs().max()) * 2)
    mod.weight.grad.zero_()
    mod.bias.grad.zero_()
    y = linear(mod, x, activation='relu')
    for g, w in zip(gs, want):
        dx, = torch.autograd.grad(y, [x], g, retain_graph=True)
        _close(dx, w[0], 1e-5 * float(w[0].abs().max()))
    L.sync_deferred()
    torch.cuda.synchronize()
    for got, a, b in zip((mod.weight.grad, mod.bias.grad), want[0][1:], want[1][1:]):
        _close(got, a + b, 1e-5 * float((a + b).abs().max()))


# -------------------------------------------------------------------------------------------------------------------- losses
def test_pit_fused_review_second_backward():
    """``pit_mse_ips_losses`` (ragged batch, device lengths) against the oracle's python-loop ``pit_loss`` in fp64 (``pit/model.py:117-140``)."""
    from oracle import torch_ref
    from padertorch_amd.ops.losses.source_separation import pit_mse_ips_losses
    torch.manual_seed(13)
    B, T, K, F = 4, 9, 2, 33
    lens = [9, 7, 4, 1]
    mask = torch.rand(B, T, K, F, device=DEV, requires_grad=True)
    obs, tgt, cos = torch.rand(B, T, F, device=DEV), torch.rand(B, T, K, F, device=DEV), torch.rand(B, T, K, F, device=DEV) * 2 - 1
    ln = torch.tensor(lens, dtype=torch.int32, device=DEV)

    def ref(m):
        mse, ips = [], []
        for b, n in enumerate(lens):
            est = m[b, :n] * obs[b, :n, None, :].cpu().double()
            mse.append(torch_ref.pit_loss(est, tgt[b, :n].cpu().double(), axis=-2))
            ips.append(torch_ref.pit_loss(est, (tgt[b, :n] * cos[b, :n]).cpu().double(), axis=-2))
        return torch.stack([torch.stack(mse).mean(), torch.stack(ips).mean()])
    gs = [torch.tensor([0.25, 1.], device=DEV), torch.tensor([-1.3, 0.6], device=DEV)]
    _twice(lambda m: pit_mse_ips_losses(m, obs, tgt, cos, ln)[0], [mask], ref, gs, lambda w: (1e-7, 1e-4))


def test_pit_loss_second_backward():
    from oracle import torch_ref
    from padertorch_amd.ops.losses.source_separation import pit_loss
    torch.manual_seed(14)
    est = torch.randn(11, 3, 17, device=DEV, requires_grad=True)
    tgt = torch.randn(11, 3, 17, device=DEV)
    gs = [torch.tensor(1., device=DEV), torch.tensor(-0.37, device=DEV)]
    _twice(lambda e: pit_loss(e, tgt, axis=-2), [est], lambda e: torch_ref.pit_loss(e, tgt.cpu().double(), axis=-2), gs,
           lambda w: (1e-7, 1e-4))


@pytest.mark.parametrize('E,K', [(8, 3), (30, 3)])
def test_deep_clustering_loss_second_backward(E, K):
    """``deep_clustering_loss``: the Gram kernel (E + K <= 32) and the planes-GEMM form beyond, against the oracle's in fp64."""
    from oracle import torch_ref
    from padertorch_amd.ops.losses.source_separation import deep_clustering_loss
    torch.manual_seed(E)
    N = 300
    x = torch.nn.functional.normalize(torch.randn(N, E), dim=1).to(DEV).requires_grad_(True)
    t = torch.nn.functional.one_hot(torch.randint(0, K, (N,)), K).float().to(DEV)
    gs = [torch.tensor(1., device=DEV), torch.tensor(-2.5, device=DEV)]
    _twice(lambda x: deep_clustering_loss(x, t), [x], lambda x: torch_ref.deep_clustering_loss(x, t.cpu().double()), gs, _rel(1e-5))


def test_dc_loss_batched_second_backward():
    """The fused ragged deep-clustering review (``contrib/tcl/dc.py:73-84``) against the oracle's per-example loss in fp64."""
    from oracle import torch_ref
    from padertorch_amd.ops.losses.source_separation import dc_loss_batched
    torch.manual_seed(15)
    T, B, E, K, F = 7, 3, 6, 2, 9
    lens = [7, 5, 2]
    emb = torch.nn.functional.normalize(torch.randn(T, B, E, F), dim=2).to(DEV).requires_grad_(True)
    tm = torch.nn.functional.one_hot(torch.randint(0, K, (B, T, F)), K).permute(0, 1, 3, 2).float().contiguous().to(DEV)
    ln = torch.tensor(lens, dtype=torch.int32, device=DEV)

    def ref(e):
        losses = []
        for b, n in enumerate(lens):
            x = e[:n, b].permute(0, 2, 1).reshape(-1, E)
            t = tm[b, :n].cpu().double().permute(0, 2, 1).reshape(-1, K)
            losses.append(torch_ref.deep_clustering_loss(x, t))
        return torch.stack(losses).mean()
    gs = [torch.tensor(1., device=DEV), torch.tensor(0.3, device=DEV)]
    _twice(lambda e: dc_loss_batched(e, tm, ln)[0], [emb], ref, gs, _rel(1e-5))


def test_time_domain_losses_second_backward():
    """``ops.losses.regression`` (five fp64 sums per pair from one HIP pass, the gradient from a second): SI-SDR of [B, K, T] rows
    (``regression.py:178-296``) against its closed form in fp64 - gradients w.r.t. the estimate AND the target."""
    from padertorch_amd.ops.losses import regression as R
    torch.manual_seed(16)
    e = torch.randn(3, 2, 200, device=DEV, requires_grad=True)
    t = torch.randn(3, 2, 200, device=DEV, requires_grad=True)

    def ref(e, t):
        alpha = (e * t).sum(-1, keepdim=True) / (t * t).sum(-1, keepdim=True)
        s = alpha * t
        return -(10 * torch.log10((s * s).sum(-1) / ((e - s) ** 2).sum(-1))).mean()
    gs = [torch.tensor(1., device=DEV), torch.tensor(-0.7, device=DEV)]
    _twice(lambda e, t: R.si_sdr_loss(e, t), [e, t], ref, gs, lambda w: (2e-6 * max(1., float(w.abs().max())), 2e-4))


# ---------------------------------------------------------------------------------------------------------------- other ops
def test_unit_norm_second_backward():
    from padertorch_amd.ops import unit_norm
    torch.manual_seed(17)
    for E in (8, 40):                      # register-tiled kernel, two-read kernel
        x = torch.randn(5, E, 13, device=DEV, requires_grad=True)
        gs = [torch.randn(5, E, 13, device=DEV) for _ in range(2)]
        _twice(unit_norm, [x], lambda x: torch.nn.functional.normalize(x, dim=-2), gs, lambda w: (1e-5, 1e-5))


def test_stft_second_backward():
    """``STFT.__call__`` (its backward is the adjoint, an inverse-STFT kernel) against the reference's conv1d STFT in fp64."""
    from oracle import torch_ref
    from padertorch_amd.ops import STFT
    torch.manual_seed(18)
    st = STFT(512, 128, complex_representation='concat')
    conv = torch_ref.ConvSTFT(512, 128)
    x = (0.1 * torch.randn(2, 3000)).to(DEV).requires_grad_(True)

    def ref(x):
        z = conv(x)
        return torch.cat([z.real, z.imag], -1)
    frames = ref(x.detach().cpu().double()).shape[-2]
    gs = [torch.randn(2, frames, 514, device=DEV) for _ in range(2)]
    _twice(st, [x], ref, gs, _rel(2e-5))


def test_pick_second_backward():
    """``ops.scalars.pick`` hands autograd a cached one-hot vector: two passes accumulate, and neither changes the cache."""
    from padertorch_amd.ops.scalars import pick, unit_grad
    v = torch.randn(4, device=DEV, requires_grad=True)
    out = pick(v, 2)
    one = unit_grad(out)
    torch.autograd.backward(out, one, retain_graph=True)
    torch.autograd.backward(out, one, retain_graph=True)
    assert v.grad.tolist() == [0., 0., 2., 0.]
    assert torch.autograd.grad(out, v, one, retain_graph=True)[0].tolist() == [0., 0., 1., 0.]
    assert torch.autograd.grad(out, v, torch.tensor(-3., device=DEV), retain_graph=True)[0].tolist() == [0., 0., -3., 0.]
    assert pick(v, 2).backward(one) is None and v.grad.tolist() == [0., 0., 3., 0.]
