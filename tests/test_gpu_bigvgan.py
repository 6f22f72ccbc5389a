"""The BigVGAN generator on the GPU: the convolution kernels of csrc/bigvgan.hip one by one, on both paths and through every epilogue,
and the whole generator against the reference's fp64 golden runs (tests/golden/g23_bigvgan.npz).

Gate, for every quantity ``q``: ``max|q - q64| / max|q64| <= max(4 dev32, 4 * 2^-23)`` - the convention of tests/test_gpu_anti_alias.py -
with ``dev32`` the fp32 deviation of the reference itself from its fp64 run on the same data: from the golden for the generator, taken
here from torch's fp32 CPU convolution against its fp64 one for the single kernels.  Every deviation is printed next to its gate
(``GATE`` lines; profiles/bigvgan_gates.txt holds a copy)."""
import json

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import bigvgan_ref as ref

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def ops():
    from padertorch_amd.ops import bigvgan
    return bigvgan


def bigvgan():
    from padertorch_amd.contrib.mk.synthesis.vocoder import nvidia_bigvgan
    return nvidia_bigvgan


def check(label, got, want64, got32):
    """``got`` (GPU) against ``want64`` under the gate of ``got32``, the reference's own fp32 result; returns (deviation, gate)."""
    dev32 = ref.rel_dev(got32, want64)
    dev, gate = ref.rel_dev(got, want64), ref.gate(dev32)
    print(f'GATE {label:58s} deviation {dev:.3g}  gate {gate:.3g}  (dev32 {dev32:.3g})')
    assert dev <= gate, (label, dev, gate)
    return dev, gate


# ------------------------------------------------------------------------------------------------------------ conv1d
def conv_shapes():
    o = ops()
    return [(3, 5, 3, 1, 1, True), (8, 8, 11, 5, 7, True), (24, 24, 7, 3, o.DIRECT_TILE + 1, True), (24, 24, 7, 3, o.TAPS_TILE + 1, True),
            (o.DIRECT_MAX_CHANNELS, 16, 11, 1, 40, True), (130, 70, 3, 5, 300, False)]


def conv_reference(x, w, b, d, residual, out0, scale, dtype):
    K = w.shape[2]
    y = F.conv1d(x.to(dtype), w.to(dtype), b.to(dtype), dilation=d, padding=(K - 1) * d // 2)
    if residual is not None:
        y = y + residual.to(dtype)
    y = y * torch.tensor(scale, dtype=dtype)
    return y if out0 is None else out0.to(dtype) + y


@pytest.mark.parametrize('index', range(6))
def test_conv1d_on_both_paths(index):
    c_in, c_out, K, d, T, direct = conv_shapes()[index]
    o = ops()
    assert o.direct_ok(c_in, K, d) == direct
    rs = np.random.RandomState(100 + index)
    B = 2

    def rand(*shape, s=1.0):
        return torch.from_numpy((s * rs.randn(*shape)).astype(np.float32))
    x, w, b = rand(B, c_in, T), rand(c_out, c_in, K, s=(c_in * K) ** -0.5), rand(c_out, s=0.1)
    residual, out0 = rand(B, c_out, T), rand(B, c_out, T)
    variants = {'plain': (None, None, 1.0), 'residual': (residual, None, 1.0), 'accumulate': (residual, out0, 1.0 / 3)}
    for name, (res, o0, scale) in variants.items():
        want = conv_reference(x, w, b, d, res, o0, scale, torch.float64)
        got32 = conv_reference(x, w, b, d, res, o0, scale, torch.float32)
        got = {}
        for path in ('gemm', 'direct') if direct else ('gemm',):
            out = None if o0 is None else o0.to(DEV).clone()
            y = o.conv1d(x.to(DEV), w.to(DEV), b.to(DEV), d, residual=None if res is None else res.to(DEV), out=out,
                         accumulate=o0 is not None, scale=scale, path=path)
            assert out is None or y is out
            assert y.shape == want.shape and y.dtype == torch.float32
            got[path] = (y, check(f'conv1d {(c_in, c_out, K, d, T)} {name} {path}', y, want, got32))
        if direct:                                           # the two paths agree within the sum of their gates
            between = float((got['gemm'][0].double() - got['direct'][0].double()).abs().max()) / float(want.abs().max())
            print(f'GATE conv1d {(c_in, c_out, K, d, T)} {name} gemm against direct: {between:.3g}')
            assert between <= got['gemm'][1][1] + got['direct'][1][1]
    # the automatic choice is one of the two and gives its bits
    auto = o.conv1d(x.to(DEV), w.to(DEV), b.to(DEV), d)
    path = o.choose_path(c_in, K, d)
    assert torch.equal(auto, o.conv1d(x.to(DEV), w.to(DEV), b.to(DEV), d, path=path))


def test_conv1d_direct_above_its_limits_raises():
    o = ops()
    wide = o.DIRECT_MAX_CHANNELS + 1
    with pytest.raises(ValueError, match='direct'):
        o.conv1d(torch.zeros(1, wide, 9, device=DEV), torch.zeros(2, wide, 3, device=DEV), path='direct')
    assert o.choose_path(wide, 3, 1) == 'gemm'
    y = o.conv1d(torch.zeros(1, wide, 9, device=DEV), torch.ones(2, wide, 3, device=DEV), torch.ones(2, device=DEV))
    assert torch.equal(y, torch.ones_like(y))                # the automatic choice goes to the GEMM path (all-zero input: the bias is left)


# ------------------------------------------------------------------------------------------------------------ conv_transpose1d
@pytest.mark.parametrize('u,k', [(2, 4), (4, 8), (8, 16), (3, 7), (2, 5), (1, 1)])
def test_conv_transpose1d(u, k):
    o = ops()
    rs = np.random.RandomState(200 + 10 * u + k)
    for c_in, c_out in ((6, 3), (70, 35)):
        w = torch.from_numpy((rs.randn(c_in, c_out, k) * (c_in * k) ** -0.5).astype(np.float32))
        b = torch.from_numpy((0.1 * rs.randn(c_out)).astype(np.float32))
        for T in (1, 5, 130):
            x = torch.from_numpy(rs.randn(2, c_in, T).astype(np.float32))
            want = F.conv_transpose1d(x.double(), w.double(), b.double(), stride=u, padding=(k - u) // 2)
            got32 = F.conv_transpose1d(x, w, b, stride=u, padding=(k - u) // 2)
            assert want.shape[-1] == (T - 1) * u - 2 * ((k - u) // 2) + k
            y = o.conv_transpose1d(x.to(DEV), w.to(DEV), b.to(DEV), u)
            assert y.shape == want.shape
            check(f'conv_transpose1d u {u} k {k} {c_in}->{c_out} T {T}', y, want, got32)
            assert ref.rel_dev(ref.conv_transpose1d(x.double(), w.double(), b.double(), u), want) <= 1e-12
    y0 = o.conv_transpose1d(x.to(DEV), w.to(DEV), None, u)
    assert ref.rel_dev(y0, want - b.double().view(1, -1, 1)) <= ref.gate(ref.rel_dev(got32, want))


# ------------------------------------------------------------------------------------------------------------ conv_post
@pytest.mark.parametrize('C', [1, 12, 70])
def test_conv_post(C):
    o = ops()
    rs = np.random.RandomState(300 + C)
    w = torch.from_numpy((rs.randn(1, C, 7) * (C * 7) ** -0.5).astype(np.float32))
    for T in (1, 300):
        x = torch.from_numpy((1.5 * rs.randn(2, C, T)).astype(np.float32))          # |conv| passes 1 here and there: the clamp acts
        for bias in (None, torch.tensor([0.2])):
            lin64 = F.conv1d(x.double(), w.double(), None if bias is None else bias.double(), padding=3)
            lin32 = F.conv1d(x, w, bias, padding=3)
            for tanh in (True, False):
                want = torch.tanh(lin64) if tanh else lin64.clamp(-1, 1)
                got32 = torch.tanh(lin32) if tanh else lin32.clamp(-1, 1)
                y = o.conv_post(x.to(DEV), w.to(DEV), None if bias is None else bias.to(DEV), tanh=tanh)
                assert tuple(y.shape) == (2, 1, T)
                check(f'conv_post C {C} T {T} bias {bias is not None} {"tanh" if tanh else "clamp"}', y, want, got32)
                assert float(y.abs().max()) <= 1.0
        if T == 300:
            assert float(lin64.abs().max()) > 1.0 or C == 1
    # a NaN sample comes out as NaN at exactly the 7 outputs it touches, under tanh and under the clamp
    for T, t0 in ((300, 100), (300, 1), (1, 0)):
        x = torch.from_numpy(rs.randn(2, C, T).astype(np.float32))
        x[1, C // 2, t0] = float('nan')
        for tanh in (True, False):
            y = o.conv_post(x.to(DEV), w.to(DEV), torch.tensor([0.2], device=DEV), tanh=tanh).cpu()
            expect = torch.zeros(2, 1, T, dtype=torch.bool)
            expect[1, 0, max(0, t0 - 3):t0 + 4] = True
            assert torch.equal(torch.isnan(y), expect), (C, T, t0, tanh)


# ------------------------------------------------------------------------------------------------------------ generator
def model_of(name):
    meta, x, want, dev32 = ref.case(name)
    m = bigvgan().BigVGAN(meta['h'])
    m.load_state_dict(ref.state(name), strict=True)
    return meta, x, want, dev32, m.to(DEV).eval()


def trace(model, x):
    """``dict(y, pre, up<i>, mean<i>)`` of ``model(x)``: the intermediates through hooks, as tests/golden/make_golden_bigvgan.py takes them."""
    got = {}
    hooks = [model.conv_pre.register_forward_hook(lambda m, a, o: got.__setitem__('pre', o.clone()))]
    n = len(model.ups)
    for i in range(n):
        hooks.append(model.ups[i][0].register_forward_hook(lambda m, a, o, i=i: got.__setitem__(f'up{i}', o.clone())))
        after = model.ups[i + 1][0] if i + 1 < n else model.activation_post
        hooks.append(after.register_forward_pre_hook(lambda m, a, i=i: got.__setitem__(f'mean{i}', a[0].clone())))
    with torch.no_grad():
        got['y'] = model(x)
    for hk in hooks:
        hk.remove()
    return got


def check_case(label, got, want, dev32, quantities):
    failed = []
    for q in quantities:
        d32 = dev32.get(q, dev32['y'])
        dev, gate = ref.rel_dev(got[q], want[q]), ref.gate(d32)
        print(f'GATE {label:28s} {q:6s} deviation {dev:.3g}  gate {gate:.3g}  (dev32 {d32:.3g})')
        if not dev <= gate:
            failed.append((q, dev, gate))
    assert not failed, (label, failed)


@pytest.mark.parametrize('name', ref.case_names())
def test_golden_case(name):
    meta, x, want, dev32, m = model_of(name)
    got = trace(m, x.to(DEV))
    assert list(got['y'].shape) == meta['out_shape'] and set(got) == set(want)
    check_case(name, got, want, dev32, meta['quantities'])


def test_state_dict_round_trip():
    meta, x, want, dev32, m = model_of('amp2')
    state = {k: v.cpu() for k, v in m.state_dict().items()}
    assert all(torch.equal(v, ref.state('amp2')[k]) for k, v in state.items())
    m2 = bigvgan().BigVGAN(meta['h'])
    m2.load_state_dict(state, strict=True)
    with torch.no_grad():
        assert torch.equal(m2.to(DEV)(x.to(DEV)), m(x.to(DEV)))


@pytest.mark.parametrize('path', ['gemm', 'direct'])
def test_generator_with_every_convolution_on_one_path(path):
    meta, x, want, dev32, m = model_of('amp1')
    m.conv_path = path
    check_case(f'amp1 all {path}', trace(m, x.to(DEV)), want, dev32, meta['quantities'])


def test_weight_normed_checkpoint_gives_the_folded_models_output():
    meta, x, want, dev32, m = model_of('k1')
    m2 = bigvgan().BigVGAN(meta['h'])
    m2.load_state_dict(ref.state('k1', 'sd_wn'), strict=True)
    check_case('k1 from weight_g / weight_v', trace(m2.to(DEV).eval(), x.to(DEV)), want, dev32, meta['quantities'])


def test_eager_calls_and_a_replayed_graph_give_the_same_bits():
    meta, x, want, dev32, m = model_of('amp1')
    x1 = x.to(DEV)
    x2 = torch.from_numpy(np.random.RandomState(7).randn(*x.shape).astype(np.float32)).to(DEV) * 0.5
    with torch.no_grad():
        a, b = m(x1), m(x1)
        assert torch.equal(a, b)
        eager2 = m(x2)
        assert not torch.equal(a, eager2)
        static_x = x1.clone()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            m(static_x)
        torch.cuda.current_stream().wait_stream(side)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            static_y = m(static_x)
        graph.replay()
        assert torch.equal(static_y, a)
        static_x.copy_(x2)
        graph.replay()
        assert torch.equal(static_y, eager2)
        static_x.copy_(x1)
        graph.replay()
        assert torch.equal(static_y, a)
        assert torch.equal(m(x2), eager2)                    # and the eager path is untouched by the capture
    torch.cuda.synchronize()


def test_vocoder(tmp_path):
    from padertorch_amd.contrib.mk.synthesis.vocoder import Vocoder
    meta, x, want, dev32, m = model_of('amp1')
    d = tmp_path / 'bigvgan_v2_24khz_8band_8x'
    d.mkdir()
    (d / 'config.json').write_text(json.dumps(meta['h']))
    torch.save({'generator': ref.state('amp1')}, d / 'bigvgan_generator.pt')
    v = Vocoder(base_dir=tmp_path, sampling_rate=24000, mel_bands=8, upsampling_ratio=8, device=DEV)
    assert v.sampling_rate == 24000
    xg = x.to(DEV)
    with torch.no_grad():
        whole = [m(xg[b:b + 1]).view(-1) for b in range(2)]
        cut = m(xg[1:2, :, :5]).view(-1)
    # 2-D: [features, time] -> [T]
    y = v(xg[0])
    assert isinstance(y, torch.Tensor) and y.shape == (72,) and torch.equal(y, whole[0])
    check_case('vocoder 2-D', {'y': y.view(1, 1, -1)}, {'y': want['y'][:1]}, dev32, ['y'])
    # 3-D, equal lengths: [batch, T]
    y = v(xg)
    assert isinstance(y, torch.Tensor) and y.shape == (2, 72) and torch.equal(y[0], whole[0]) and torch.equal(y[1], whole[1])
    # lengths that differ: a list, each entry the generator on the cut input
    y = v(xg, sequence_lengths=[9, 5])
    assert isinstance(y, list) and len(y) == 2 and torch.equal(y[0], whole[0]) and y[1].shape == (40,) and torch.equal(y[1], cut)
    # numpy in, numpy out
    y = v(x.numpy())
    assert isinstance(y, np.ndarray) and y.dtype == np.float32 and y.shape == (2, 72) and np.array_equal(y[1], whole[1].cpu().numpy())
    y = v(x[0].numpy())
    assert isinstance(y, np.ndarray) and y.shape == (72,) and np.array_equal(y, whole[0].cpu().numpy())
    y = v(x.numpy(), sequence_lengths=[9, 5])
    assert isinstance(y, list) and all(isinstance(s, np.ndarray) for s in y) and np.array_equal(y[1], cut.cpu().numpy())
    # other axes: [time, batch, features]
    v2 = Vocoder(base_dir=tmp_path, vocoder_tag=d.name, device=DEV, batch_axis=1, sequence_axis=0, postprocessing=lambda s: 2 * s)
    y = v2(xg.permute(2, 0, 1))
    assert y.shape == (2, 72) and torch.equal(y[1], 2 * whole[1])
    with pytest.raises(NotImplementedError, match='resampl'):
        v(xg[0], target_sampling_rate=16000)
