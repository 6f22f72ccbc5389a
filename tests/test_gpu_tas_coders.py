"""TasEncoder / TasDecoder / TasDecoder.masked on the HIP kernels (csrc/tas_coders.hip) against the reference's fp64 results
(tests/golden/g13_tas_coders.npz) and torch's fp64 convolutions on the CPU.

Gates (the issue's, the project's own of tests/test_gpu_td.py): values |diff| <= 1e-5 max|want|, gradients |diff| <= 2e-4 max|want|.
The reference's own fp32 run differs from fp64 by at most 1.0e-6 max|want| on these tensors, so a differently ordered fp32 sum has
ten times that room in the values.  Every comparison prints its ratio diff / (gate max|want|)  (run with -s; profiles/tas_coders.txt)."""
import importlib.util
import json
from pathlib import Path

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

GOLDEN = Path(__file__).resolve().parent / 'golden'
VALUE, GRAD = 1e-5, 2e-4


@pytest.fixture(scope='module')
def g13():
    d = dict(np.load(GOLDEN / 'g13_tas_coders.npz', allow_pickle=False))
    d['cases'] = json.loads(str(d['cases']))
    spec = importlib.util.spec_from_file_location('make_golden_tas_coders', GOLDEN / 'make_golden_tas_coders.py')
    d['maker'] = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(d['maker'])             # for inputs(): the seeded x, masks and r (the reference is not imported)
    return d


def close(name, got, want, gate, every=1):
    got = got.detach().double().cpu().reshape(-1)[::every]
    want = torch.as_tensor(np.asarray(want)).double().reshape(-1)
    assert got.shape == want.shape, (name, got.shape, want.shape)
    ratio = float((got - want).abs().max() / (gate * want.abs().max()))
    print(f'tas_coders ratio {name}: {ratio:.4f} of the gate {gate:g}')
    assert ratio <= 1.0, (name, ratio)
    return ratio


def coders(L, N, stride, bias, seed=0):
    from padertorch_amd.contrib.examples.source_separation.tasnet import TasDecoder, TasEncoder
    torch.manual_seed(seed)
    kw = dict(window_length=L, feature_size=N, stride=stride, bias=bias)
    return TasEncoder(**kw).cuda(), TasDecoder(**kw).cuda()


def chain(enc, dec, x, mask, r, fused=True):
    """encode -> masked decode -> sum(y r) -> backward.  Returns values and gradients as a dict."""
    params = [p for p in list(enc.parameters()) + list(dec.parameters())]
    x, mask = x.detach().requires_grad_(), mask.detach().requires_grad_()
    w, _ = enc(x)
    y = dec.masked(mask, w) if fused else dec((mask * w[None]).flatten(0, 1)).view(mask.shape[0], w.shape[0], -1)
    grads = torch.autograd.grad((y * r).sum(), [x, mask] + params)
    names = ['x', 'mask', 'enc_weight'] + (['enc_bias'] if enc.encoder_1d.bias is not None else []) + ['dec_weight'] \
        + (['dec_bias'] if dec.decoder_1d.bias is not None else [])
    return dict(encoded=w.detach(), tail=y.detach(), **{'g_' + n: g for n, g in zip(names, grads)})


def chain_fp64(enc, dec, x, mask, r):
    """The same chain with torch's convolutions in fp64 on the CPU (explicit padding to a multiple of half a window)."""
    L, s = enc.window_length, enc.stride
    par = {k: v.detach().double().cpu().requires_grad_() for k, v in list(enc.state_dict().items()) + list(dec.state_dict().items())}
    x, mask, r = x.detach().double().cpu().requires_grad_(), mask.detach().double().cpu().requires_grad_(), r.double().cpu()
    h = L // 2
    xp = F.pad(x, (0, (h - x.shape[1] % h) % h))
    w = F.relu(F.conv1d(xp[:, None], par['encoder_1d.weight'], par.get('encoder_1d.bias'), stride=s))
    y = F.conv_transpose1d((mask * w[None]).flatten(0, 1), par['decoder_1d.weight'], par.get('decoder_1d.bias'), stride=s)[:, 0]
    y = y.view(mask.shape[0], x.shape[0], -1)
    decoded = F.conv_transpose1d(w, par['decoder_1d.weight'], par.get('decoder_1d.bias'), stride=s)[:, 0].detach()
    (y * r).sum().backward()
    out = dict(encoded=w.detach(), tail=y.detach(), decoded=decoded, g_x=x.grad, g_mask=mask.grad)
    out.update({'g_' + k.replace('encoder_1d.', 'enc_').replace('decoder_1d.', 'dec_'): v.grad for k, v in par.items()})
    return out


@pytest.mark.parametrize('index', range(5))
def test_fixture_geometries_match_the_reference_fp64(g13, index):
    case = g13['cases'][index]
    L, N, stride, bias, T = case
    p = f'c{index}_'
    enc, dec = coders(L, N, stride, bias)
    enc.load_state_dict({k.replace(p + 'enc_', 'encoder_1d.'): torch.from_numpy(v) for k, v in g13.items() if k.startswith(p + 'enc_')})
    dec.load_state_dict({k.replace(p + 'dec_', 'decoder_1d.'): torch.from_numpy(v) for k, v in g13.items() if k.startswith(p + 'dec_')})
    shapes = g13[p + 'shapes']
    x, mask, r = (torch.from_numpy(a).cuda() for a in g13['maker'].inputs(index, case, int(shapes[0][2]), int(shapes[1][1])))
    w, lengths = enc(x, torch.from_numpy(g13[p + 'lengths_in']))
    assert tuple(w.shape) == tuple(shapes[0]) and lengths.tolist() == g13[p + 'lengths_out'].tolist()
    assert enc(x)[1] is None
    got = chain(enc, dec, x, mask, r)
    close(f'{case} encoded', got['encoded'], g13[p + 'encoded'], VALUE, int(g13[p + 'encoded_every']))
    close(f'{case} decoded', dec(w), g13[p + 'decoded'], VALUE)
    close(f'{case} tail', got['tail'], g13[p + 'tail'], VALUE)
    close(f'{case} g_mask', got['g_mask'], g13[p + 'g64_mask'], GRAD, int(g13[p + 'g64_mask_every']))
    for name in ['x', 'enc_weight', 'dec_weight'] + (['enc_bias', 'dec_bias'] if bias else []):
        close(f'{case} g_{name}', got['g_' + name], g13[p + 'g64_' + name], GRAD)


#: (B, T, L, N, stride, K, bias): the three sizes of the reference's configurations, the odd ones, stride > L, and one per path the
#: kernels switch to: L > 32 and K > 4 (generic analysis, two mask groups), N L > 12288 (synthesis weights not in LDS), a stride whose
#: signal segment does not fit the weight-gradient kernel's LDS, feature rows split between two of its workgroups (L = 3, N L > 256)
FULL = [(4, 32000, 16, 64, 8, 2, False), (1, 8000, 2, 64, 1, 2, False), (2, 16000, 20, 256, 10, 2, True), (3, 1001, 16, 32, 4, 3, True),
        (2, 203, 5, 7, 3, 2, True), (2, 300, 4, 5, 6, 2, True), (2, 3000, 40, 9, 13, 5, True), (1, 9000, 6, 3, 700, 2, True),
        (1, 640, 32, 400, 16, 1, False), (2, 700, 3, 130, 1, 4, True)]


@pytest.mark.parametrize('cfg', FULL, ids=lambda c: 'x'.join(map(str, c)))
def test_against_fp64_convolutions_and_the_unfused_composition(cfg):
    B, T, L, N, stride, K, bias = cfg
    enc, dec = coders(L, N, stride, bias, seed=1)
    gen = torch.Generator().manual_seed(7)
    x = torch.randn(B, T, generator=gen).cuda()
    frames = enc(x)[0].shape[2]
    mask = torch.rand(K, B, N, frames, generator=gen).cuda()
    r = torch.randn(K, B, (frames - 1) * stride + L, generator=gen).cuda()
    want = chain_fp64(enc, dec, x, mask, r)
    got = chain(enc, dec, x, mask, r)
    unfused = chain(enc, dec, x, mask, r, fused=False)
    assert set(got) == set(unfused) == set(want) - {'decoded'}
    for k, v in got.items():
        gate = GRAD if k.startswith('g_') else VALUE
        close(f'{cfg} {k}', v, want[k], gate)
        close(f'{cfg} {k} unfused', unfused[k], want[k], gate)
        close(f'{cfg} {k} fused vs unfused', v, unfused[k].double().cpu(), gate)
    close(f'{cfg} decoded', dec(got['encoded']), want['decoded'], VALUE)


@pytest.mark.parametrize('L, N, stride', [(16, 64, 8), (20, 32, 7), (4, 5, 6), (40, 6, 9)])
def test_analysis_and_synthesis_are_adjoint(L, N, stride):
    from padertorch_amd import ops
    gen = torch.Generator().manual_seed(3)
    E = 777
    T = (E - 1) * stride + L
    W = torch.randn(N, 1, L, generator=gen).cuda()
    v, u = torch.randn(3, T, generator=gen).cuda(), torch.randn(3, N, E, generator=gen).cuda()
    av = torch.ops.ptmi.tas_analysis(v, W, None, stride, E, False)             # the encoder without its ReLU
    su = ops.tas_decode(u, W, None, stride)
    lhs, rhs = float((av.double() * u.double()).sum()), float((v.double() * su.double()).sum())
    print(f'tas_coders adjoint L={L} N={N} s={stride}: {lhs:.9g} vs {rhs:.9g}')
    assert abs(lhs - rhs) <= 2e-4 * abs(rhs)


def test_implicit_padding_is_bit_identical_to_explicit_padding():
    enc, _ = coders(16, 24, None, True)
    x = torch.randn(2, 1003, generator=torch.Generator().manual_seed(5)).cuda().requires_grad_()
    xp = F.pad(x.detach(), (0, 5)).requires_grad_()             # 1003 -> 1008, the next multiple of 8
    w, wp = enc(x)[0], enc(xp)[0]
    assert w.shape == wp.shape == (2, 24, 125) and torch.equal(w, wp)
    g = torch.randn(w.shape, generator=torch.Generator().manual_seed(6)).cuda()
    (gx,), (gxp,) = torch.autograd.grad(w, x, g), torch.autograd.grad(wp, xp, g)
    assert gx.shape == (2, 1003) and torch.equal(gx, gxp[:, :1003])
    w1, lengths = enc(x.detach()[0], torch.tensor([1003]))
    assert w1.shape == (1, 24, 125) and torch.equal(w1[0], w[0]) and lengths.tolist() == [125]


def _fixed_inputs(seed, B=2, T=4001, N=32, frames=500, K=2, samples=4008):          # L 16, stride 8: 4001 -> 4008 samples, 500 frames
    gen = torch.Generator().manual_seed(seed)
    return (torch.randn(B, T, generator=gen).cuda(), torch.rand(K, B, N, frames, generator=gen).cuda(),
            torch.randn(K, B, samples, generator=gen).cuda())


def test_runs_are_bit_identical_and_capturable():
    enc, dec = coders(16, 32, None, True)
    x, mask, r = _fixed_inputs(11)
    first, second = chain(enc, dec, x, mask, r), chain(enc, dec, x, mask, r)
    for k in first:
        assert torch.equal(first[k], second[k]), k
    sx, sm, sr = x.clone(), mask.clone(), r.clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        chain(enc, dec, sx, sm, sr)                                # eager warm-up on the capture stream
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        captured = chain(enc, dec, sx, sm, sr)
    for seed in (12, 13):
        x, mask, r = _fixed_inputs(seed)
        sx.copy_(x), sm.copy_(mask), sr.copy_(r)
        graph.replay()
        torch.cuda.synchronize()
        eager = chain(enc, dec, x, mask, r)
        for k in eager:
            assert torch.equal(captured[k], eager[k]), (seed, k)


def test_non_contiguous_inputs():
    enc, dec = coders(16, 32, None, False)
    x, mask, r = _fixed_inputs(21)
    wide = torch.randn(2, 2 * 4001 + 3, generator=torch.Generator().manual_seed(22)).cuda()
    wide[:, 3::2] = x
    x_nc = wide[:, 3::2]
    mask_nc = mask.permute(0, 1, 3, 2).contiguous().permute(0, 1, 3, 2)
    assert not x_nc.is_contiguous() and not mask_nc.is_contiguous() and torch.equal(mask_nc, mask)
    a, b = chain(enc, dec, x, mask, r), chain(enc, dec, x_nc, mask_nc, r)
    for k in a:
        assert torch.equal(a[k], b[k]), k
    enc_t = enc(x)[0].transpose(1, 2).contiguous().transpose(1, 2)
    assert torch.equal(dec(enc_t), dec(enc(x)[0]))


def test_other_dtypes_are_refused():
    enc, dec = coders(16, 8, None, False)
    with pytest.raises(NotImplementedError, match='float32'):
        enc(torch.zeros(1, 64, device='cuda', dtype=torch.float64))
    with pytest.raises(NotImplementedError, match='float32'):
        dec(torch.zeros(1, 8, 7, device='cuda', dtype=torch.float16))
