"""The WaveNet vocoder on the GPU: the kernels of csrc/wavenet.hip against the reference's fp64 golden run (tests/golden/g22_wavenet.npz)
and, at shapes the fixture does not hold, against the fp64 restatement (tests/wavenet_ref.py).

Gates: ``VALUE = 1e-5`` for values and ``GRAD = 2e-4`` for gradients, times ``max|want|``, against fp64 (the reference's own fp32 run
deviates by 2.0e-7 / at most 7.5e-7 in the fixture - below a quarter of either gate, asserted by the fixture's maker).  Every comparison
prints its ratio to the gate (``-s``).  The sampling loop is checked against the teacher-forced fp64 logits of ITS OWN codes: the logits to
VALUE, and every draw against the fp64 CDF interval of the class it chose, widened by ``tau = 2 VALUE max|logits| + A 2^-23``."""
import pytest
import torch

import wavenet_ref as ref

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
VALUE, GRAD = ref.VALUE, ref.GRAD


def wn():
    from padertorch_amd.ops import wavenet
    return wavenet


def check(label, got, want, gate):
    dev = ref.rel_dev(got, want)
    print(f'{label:44s} deviation {dev:.3g}  = {dev / gate:.3g} of the gate {gate:g}')
    assert dev <= gate, (label, dev, gate)


def rand(*shape, seed, scale=1.0):
    return (torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64) * scale).float()


def one_alone(fn, inputs, weight):
    """Gradients of ``sum(fn(*inputs) * weight)`` with all inputs requiring a gradient, then with each ONE alone: the same bits."""
    def grads(which):
        leaves = [t.detach().clone().requires_grad_(i in which) for i, t in enumerate(inputs)]
        (fn(*leaves) * weight).sum().backward()
        return [t.grad for t in leaves]
    together = grads(set(range(len(inputs))))
    again = grads(set(range(len(inputs))))
    for i in range(len(inputs)):
        assert torch.equal(together[i], again[i]), f'input {i}: two runs of the backward differ'
        alone = grads({i})
        assert all(g is None for j, g in enumerate(alone) if j != i)
        assert torch.equal(alone[i], together[i]), f'input {i}: alone differs from together'
    return together


# ------------------------------------------------------------------------------------------------ 1. mu-law
def test_mu_law_against_the_reference():
    from padertorch_amd import ops
    g = ref.golden()
    x = torch.from_numpy(g['mu_x']).to(DEV)
    assert torch.equal(ops.mu_law_encode(x).cpu(), torch.from_numpy(g['mu_codes']))
    assert torch.equal(ops.mu_law_encode(x, 16).cpu(), torch.from_numpy(g['mu_codes16']))
    assert ops.mu_law_encode(x).dtype == torch.int64
    check('mu_law_decode 256', ops.mu_law_decode(torch.arange(256, device=DEV)), g['mu_decode'], VALUE)
    check('mu_law_decode 16', ops.mu_law_decode(torch.arange(16, device=DEV), 16), g['mu_decode16'], VALUE)
    check('mu_law_decode 256 (float codes)', ops.mu_law_decode(torch.arange(256, device=DEV).float()), g['mu_decode'], VALUE)
    bad = torch.tensor([-1.5, 0.25, 1.5], device=DEV)
    with pytest.raises(AssertionError):
        ops.mu_law_encode(bad)
    assert ops.mu_law_encode(bad, check=False).tolist() == [0, int(ref.mu_law_encode(torch.tensor([0.25]))), 255]
    codes = torch.tensor([-3, 7, 300], device=DEV)
    with pytest.raises(AssertionError):
        ops.mu_law_decode(codes)
    assert torch.equal(ops.mu_law_decode(codes, check=False), ops.mu_law_decode(torch.tensor([0, 7, 255], device=DEV)))


# ------------------------------------------------------------------------------------------------ 2. operators alone
@pytest.mark.parametrize('R, A', [(24, 16), (64, 256)])
def test_embed(R, A):
    B, T = 2, 1300                                   # 2600 rows: three slabs of the backward's row scan, the last one partial
    audio = torch.rand((B, T), generator=torch.Generator().manual_seed(1)) * 2 - 1
    weight = rand(A, R, seed=2)
    w = rand(B, T, R, seed=3)
    x0, codes = wn().embed(audio.to(DEV), weight.to(DEV))
    want_codes = ref.mu_law_encode(audio, A)
    assert codes.dtype == torch.int64 and torch.equal(codes.cpu(), want_codes)
    assert torch.equal(x0.cpu(), weight[want_codes])
    dembed, = one_alone(lambda e: wn().embed(audio.to(DEV), e)[0], [weight.to(DEV)], w.to(DEV))
    want = torch.zeros(A, R, dtype=torch.float64).index_add_(0, want_codes.reshape(-1), w.double().reshape(-1, R))
    check(f'embed R={R} A={A}: dembed', dembed, want, GRAD)


@pytest.mark.parametrize('fading', ['full', 'half', None])
def test_cond_upsample(fading):
    B, C, Tf, window, stride = 2, 5, 12, 10, 4
    f, weight, bias = rand(B, C, Tf, seed=4), rand(C, C, window, seed=5, scale=0.3), rand(C, seed=6)
    p = {'upsample.weight': weight.double().requires_grad_(), 'upsample.bias': bias.double().requires_grad_()}
    f64 = f.double().requires_grad_()
    want = ref.upsample(p, f64, window, stride, fading).transpose(1, 2)                  # [B, Tout, C]
    w = rand(*want.shape, seed=7)
    (want * w.double()).sum().backward()

    def fn(a, b, c):
        return wn().cond_upsample(a, b, c, stride, fading)
    got = fn(f.to(DEV), weight.to(DEV), bias.to(DEV))
    check(f'cond_upsample {fading}: value', got, want.detach(), VALUE)
    got5 = wn().cond_upsample(f.to(DEV), weight.to(DEV), bias.to(DEV), stride, fading, out_len=5)
    assert torch.equal(got5, got[:, :5])
    grads = one_alone(fn, [f.to(DEV), weight.to(DEV), bias.to(DEV)], w.to(DEV))
    for name, a, b in zip(('dfeatures', 'dweight', 'dbias'), grads, (f64.grad, p['upsample.weight'].grad, p['upsample.bias'].grad)):
        check(f'cond_upsample {fading}: {name}', a, b, GRAD)


@pytest.mark.parametrize('R', [24, 64])
@pytest.mark.parametrize('d, T', [(1, 3), (4, 3), (128, 3), (4, 1), (1, 130), (4, 130), (128, 130)])
def test_gate(R, d, T):
    B, L, l = 2, 3, 1
    P, bias, wide = rand(B, T, 4 * R, seed=8), rand(2 * R, seed=9), rand(B, T, L * 2 * R, seed=10)
    w = rand(B, T, R, seed=11)

    def fp64(P, bias, cond):
        delayed = torch.nn.functional.pad(P[:, :, :2 * R], (0, 0, d, 0))[:, :T]
        z = delayed + P[:, :, 2 * R:] + bias + cond
        return torch.tanh(z[..., :R]) * torch.sigmoid(z[..., R:])
    leaves = [t.double().requires_grad_() for t in (P, bias, wide[:, :, l * 2 * R:(l + 1) * 2 * R])]
    want = fp64(*leaves)
    (want * w.double()).sum().backward()
    wide_gpu = wide.to(DEV)

    def fn(P, bias, wide):
        return wn().gate(P, bias, wide[:, :, l * 2 * R:(l + 1) * 2 * R], d)          # the conditioning is read as a slice, in place
    got = fn(P.to(DEV), bias.to(DEV), wide_gpu)
    check(f'gate R={R} d={d} T={T}: acts', got, want.detach(), VALUE)
    dP, dbias, dwide = one_alone(fn, [P.to(DEV), bias.to(DEV), wide_gpu], w.to(DEV))
    check(f'gate R={R} d={d} T={T}: dP', dP, leaves[0].grad, GRAD)
    check(f'gate R={R} d={d} T={T}: dbias', dbias, leaves[1].grad, GRAD)
    check(f'gate R={R} d={d} T={T}: dcond', dwide[:, :, l * 2 * R:(l + 1) * 2 * R], leaves[2].grad, GRAD)
    assert float(dwide[:, :, :l * 2 * R].abs().max()) == 0.0 and float(dwide[:, :, (l + 1) * 2 * R:].abs().max()) == 0.0


@pytest.mark.parametrize('R, T', [(24, 7), (64, 3)])
def test_residual_stack(R, T):
    """All layers as one operator (dilations 1, 2, 4: the last exceeds ``T = 3``): ``acts_all`` and every gradient against fp64, each
    input's gradient alone."""
    B, dil = 2, [1, 2, 4]
    L = len(dil)
    x0, cond = rand(B, T, R, seed=20), rand(B, T, L * 2 * R, seed=21)
    dw = [rand(2 * R, R, 2, seed=22 + l, scale=0.3) for l in range(L)]
    db = [rand(2 * R, seed=26 + l) for l in range(L)]
    rw = [rand(R, R, 1, seed=30 + l, scale=0.3) for l in range(L - 1)]
    rb = [rand(R, seed=34 + l) for l in range(L - 1)]
    w = rand(B, T, L, R, seed=38)
    flat = [x0, cond, *dw, *db, *rw, *rb]

    def fn(x0, cond, *p):
        return wn().residual_stack(x0, cond, dil, p[:L], p[L:2 * L], p[2 * L:3 * L - 1], p[3 * L - 1:])

    leaves = [t.double().requires_grad_() for t in flat]
    x, c64, p = leaves[0].transpose(1, 2), leaves[1].transpose(1, 2), leaves[2:]
    acts = []
    for l, d in enumerate(dil):
        z = ref.gate_z(x, p[l], p[L + l], c64[:, l * 2 * R:(l + 1) * 2 * R], d)
        acts.append(torch.tanh(z[:, :R]) * torch.sigmoid(z[:, R:]))
        if l < L - 1:
            x = x + ref.conv1x1(acts[-1], p[2 * L + l], p[3 * L - 1 + l])
    want = torch.stack(acts, 1).permute(0, 3, 1, 2)                                   # [B, T, L, R]
    (want * w.double()).sum().backward()
    check(f'residual_stack R={R} T={T}: acts_all', fn(*[t.to(DEV) for t in flat]), want.detach(), VALUE)
    grads = one_alone(fn, [t.to(DEV) for t in flat], w.to(DEV))
    for i, (g, leaf) in enumerate(zip(grads, leaves)):
        check(f'residual_stack R={R} T={T}: gradient of input {i}', g, leaf.grad, GRAD)


# ------------------------------------------------------------------------------------------------ 3. the module against the fixture
def build(cfg, params=None, seed=0):
    import padertorch_amd as pt
    torch.manual_seed(seed)
    m = pt.modules.WaveNet(cfg['C'], cfg['window'], cfg['stride'], n_in_channels=cfg['A_in'], n_layers=cfg['L'], max_dilation=cfg['max_dilation'],
                           n_residual_channels=cfg['R'], n_skip_channels=cfg['S'], n_out_channels=cfg['A'], fading=cfg['fading'])
    if params is not None:
        m.load_state_dict({k: v.float() for k, v in params.items()}, strict=True)
    return m.to(DEV)


def module_pass(m, features, audio, w):
    m.zero_grad(set_to_none=True)
    f = features.detach().requires_grad_()
    out, quantized = m(f, audio)
    (out * w).sum().backward()
    return out.detach(), quantized, f.grad, {k: p.grad for k, p in m.named_parameters()}


def test_module_against_the_reference_run():
    g = ref.golden()
    c = g['config']
    m = build(c, ref.golden_params(g))
    assert m.dilations == [1, 2, 4, 1, 2, 4, 1]
    features, audio, w = (torch.from_numpy(g[k]).to(DEV) for k in ('features', 'audio', 'w'))
    out, quantized, df, grads = module_pass(m, features, audio, w)
    assert tuple(out.shape) == (c['B'], c['A'], c['T']) and float(out[:, :, 0].abs().max()) == 0.0
    assert quantized.dtype == torch.int64 and torch.equal(quantized.cpu(), torch.from_numpy(g['quantized']))
    check('module: output', out, g['output64'], VALUE)
    check('module: dfeatures', df, g['g64_features'], GRAD)
    for name in g['names']:
        if name != 'features':
            check(f'module: d {name}', grads[name], g['g64_' + name], GRAD)
    for fading in ('full', 'half', None):
        m.fading = fading
        check(f'module: get_cond_input {fading}', m.get_cond_input(features[:1]).detach(), g['cond_' + str(fading).lower()], VALUE)


def test_module_graph_replay_is_bit_identical():
    from padertorch_amd.ops import capture
    g = ref.golden()
    m = build(g['config'], ref.golden_params(g))
    features, audio, w = (torch.from_numpy(g[k]).to(DEV) for k in ('features', 'audio', 'w'))

    def flat(res):
        out, quantized, df, grads = res
        return [out, quantized, df] + [grads[k] for k in sorted(grads)]
    eager = [t.clone() for t in flat(module_pass(m, features, audio, w))]
    for a, b in zip(eager, flat(module_pass(m, features, audio, w))):
        assert torch.equal(a, b)
    sf, sa = features.clone(), audio.clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        module_pass(m, sf, sa, w)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with capture.capture_mode():
        with torch.cuda.graph(graph, stream=side):
            capture.zero_block(sf.device)
            captured = flat(module_pass(m, sf, sa, w))
    for scale in (0.5, 1.0):
        sf.copy_(features * scale), sa.copy_(audio * scale)
        graph.replay()
        torch.cuda.synchronize()
        again = flat(module_pass(m, features * scale, audio * scale, w))
        for i, (a, b) in enumerate(zip(captured, again)):
            assert torch.equal(a, b), (scale, i)


# ------------------------------------------------------------------------------------------------ 4. full width
FULL = dict(C=8, window=10, stride=4, fading='full', A_in=256, L=16, max_dilation=128, R=64, S=256, A=256)
_FULL = {}


def full_width():
    """The full-width net, its fp64 parameters and features for 302 conditioning columns (shared by the tests below)."""
    if not _FULL:
        m, p = ref.xavier_params(FULL, 40)
        _FULL.update(m=m.to(DEV), p=p, features=rand(2, FULL['C'], 77, seed=41))
    return _FULL['m'], _FULL['p'], _FULL['features']


def test_full_width_against_the_restatement():
    m, p, features = full_width()
    B, T = 2, 300
    audio = torch.rand((B, T), generator=torch.Generator().manual_seed(42)) * 2 - 1
    w = rand(B, FULL['A'], T, seed=43)
    p64 = {k: v.clone().requires_grad_() for k, v in p.items()}
    f64 = features.double().requires_grad_()
    want, q64 = ref.forward(p64, f64, audio, FULL['window'], FULL['stride'], FULL['fading'], FULL['max_dilation'])
    (want * w.double()).sum().backward()
    out, quantized, df, grads = module_pass(m, features.to(DEV), audio.to(DEV), w.to(DEV))
    assert torch.equal(quantized.cpu(), q64)
    check('full width: output', out, want.detach(), VALUE)
    check('full width: dfeatures', df, f64.grad, GRAD)
    for name in p64:
        check(f'full width: d {name}', grads[name], p64[name].grad, GRAD)


# ------------------------------------------------------------------------------------------------ 5. infer
def check_draws(label, m, p, cfg, features, selectors, **kw):
    audio, codes, logits = m.infer(features.to(DEV), selectors=selectors.to(DEV), return_logits=True, **kw)
    codes, logits = codes.cpu(), logits.cpu()
    B, T = selectors.shape
    A = cfg['A']
    assert tuple(codes.shape) == (B, T) and tuple(logits.shape) == (B, T, A) and tuple(audio.shape) == (B, T)
    assert int(codes.min()) >= 0 and int(codes.max()) < A
    assert torch.equal(audio.cpu(), ref.mu_law_decode(codes, A).float()) or ref.rel_dev(audio, ref.mu_law_decode(codes, A)) <= VALUE
    cond = ref.cond_input(p, features.double(), cfg['window'], cfg['stride'], cfg['fading'])
    want = ref.logits_teacher_forced(p, cond, codes, cfg['max_dilation'])
    check(f'{label}: logits', logits, want, VALUE)                                                        # (a)
    lo, hi = ref.cdf_interval(want, codes)
    tau = 2 * VALUE * float(want.abs().max()) + A * 2.0 ** -23
    u = selectors.double()
    assert bool(((lo - tau < u) & (u <= hi + tau)).all()), (label, 'a draw outside its interval')         # (b)
    near = ((u - lo).abs() <= tau) | ((u - hi).abs() <= tau)
    print(f'{label}: {int(near.sum())} of {near.numel()} draws within tau = {tau:.3g} of an end of their interval')
    assert float(near.double().mean()) <= 0.10, label                                                     # (c)
    return codes, logits


SMALL = dict(C=5, window=10, stride=4, fading='half', L=7, max_dilation=4, R=24, S=40)
_SMALL = {}


def small(A):
    if A not in _SMALL:
        cfg = dict(SMALL, A=A, A_in=A)
        m, p = ref.xavier_params(cfg, 50 + A)
        _SMALL[A] = (cfg, m.to(DEV), p)
    return _SMALL[A]


@pytest.mark.parametrize('A', [16, 256])
@pytest.mark.parametrize('B', [3, 5])                   # 5: a full group of four sequences and a partial one
def test_infer_small(A, B):
    from padertorch_amd import _lib
    assert _lib.load().ptmi_wavenet_generate_ex() + 1 == 5
    cfg, m, p = small(A)
    features = rand(B, cfg['C'], 11, seed=60 + B)                                   # 11 frames, fading 'half': 44 columns
    u = torch.rand((B, 44), generator=torch.Generator().manual_seed(61 + B))
    check_draws(f'infer A={A} B={B}', m, p, cfg, features, u)


def test_infer_full_width():
    m, p, features = full_width()
    u = torch.rand((2, 302), generator=torch.Generator().manual_seed(62))           # 302 steps: the d = 128 rings wrap twice
    check_draws('infer full width', m, p, FULL, features, u)


def test_infer_one_step():
    cfg = dict(SMALL, A=16, A_in=16, window=1, stride=1, fading=None)
    m, p = ref.xavier_params(cfg, 63)
    u = torch.rand((2, 1), generator=torch.Generator().manual_seed(64))
    check_draws('infer T=1', m.to(DEV), p, cfg, rand(2, cfg['C'], 1, seed=65), u)


# ------------------------------------------------------------------------------------------------ 6. independence
@pytest.mark.parametrize('A', [16, 256])
def test_infer_sequences_are_independent(A):
    cfg, m, p = small(A)
    B = 5
    features = rand(B, cfg['C'], 11, seed=70).to(DEV)
    u = torch.rand((B, 44), generator=torch.Generator().manual_seed(71)).to(DEV)
    _, codes, logits = m.infer(features, selectors=u, return_logits=True)
    _, codes7, logits7 = m.infer(features, selectors=u, return_logits=True, steps_per_launch=7)
    assert torch.equal(codes, codes7) and torch.equal(logits, logits7)
    for b in range(B):
        _, c1, l1 = m.infer(features[b:b + 1], selectors=u[b:b + 1], return_logits=True)
        assert torch.equal(c1, codes[b:b + 1]) and torch.equal(l1, logits[b:b + 1]), b


def test_infer_full_width_launch_split_is_bit_identical():
    m, p, features = full_width()
    u = torch.rand((2, 302), generator=torch.Generator().manual_seed(72)).to(DEV)
    _, codes, logits = m.infer(features.to(DEV), selectors=u, return_logits=True)
    _, codes7, logits7 = m.infer(features.to(DEV), selectors=u, return_logits=True, steps_per_launch=129)
    assert torch.equal(codes, codes7) and torch.equal(logits, logits7)


def test_infer_chunks_and_generator():
    cfg, m, p = small(16)
    B = 3
    features = rand(B, cfg['C'], 11, seed=73).to(DEV)
    u = torch.rand((B, 44), generator=torch.Generator().manual_seed(74)).to(DEV)
    audio, codes, logits = m.infer(features, chunk_length=20, chunk_overlap=4, selectors=u, return_logits=True)
    chunks = wn().chunks_of(44, 20, 4)
    assert chunks == [(0, 19), (15, 19), (30, 14)]
    with torch.no_grad():
        cond = m._cond(features)
    parts_c, parts_l = [], []
    for i, (on, n) in enumerate(chunks):                 # every chunk as a run of its own on the slice, joined as the reference joins them
        (c, lg), = wn().generate(m.packed_weights(), m.embed.weight.detach(), cond[:, on:on + n].contiguous(), u[:, on:on + n].contiguous(),
                                 m.dilations, cfg['S'], cfg['A'], return_logits=True)
        drop = 4 if i else 0
        parts_c.append(c[:, drop:]), parts_l.append(lg[:, drop:])
    assert torch.equal(codes, torch.cat(parts_c, 1)) and torch.equal(logits, torch.cat(parts_l, 1))
    assert codes.shape[1] == 19 + 15 + 10
    from padertorch_amd import ops
    assert torch.equal(audio, ops.mu_law_decode(codes, 16))
    a1 = m.infer(features, generator=torch.Generator(DEV).manual_seed(5))
    a2 = m.infer(features, generator=torch.Generator(DEV).manual_seed(5))
    a3 = m.infer(features, generator=torch.Generator(DEV).manual_seed(6))
    assert torch.equal(a1, a2) and not torch.equal(a1, a3)
    with pytest.raises(ValueError, match='selectors'):
        m.infer(features, selectors=u[:, :43])
    with pytest.raises(ValueError, match=r'outside \[0, 1\)'):
        m.infer(features, selectors=u + 1.0)
    with pytest.raises(ValueError, match='chunk_overlap'):
        m.infer(features, chunk_length=4, chunk_overlap=4)
    # the weights are packed once per parameter version
    packed = m.packed_weights()
    assert m.packed_weights() is packed
    with torch.no_grad():
        m.conv_end.conv.weight.mul_(1.0)
    assert m.packed_weights() is not packed
