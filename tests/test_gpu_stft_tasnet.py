"""The STFT-domain TasNet (StftEncoder / IstftDecoder on the fixed-basis coder kernels, ops/stft_coders.py) against the reference's fp64
results (tests/golden/g18_stft_tasnet.npz).

Gates (the project's own, tests/test_gpu_tasnet.py): values |diff| <= 1e-5 max|want|, gradients |diff| <= 2e-4 max|want|.  On the fixture
the reference's own fp32 run differs from its fp64 run by at most these shares OF A GATE (tests/golden/make_golden_stft_tasnet.py prints
them and refuses a seed above one half): out 0.023, additional_out 0.016, the three losses 0.012, the gradients of the functional 0.021,
those of the si-sdr loss 0.013.  Every comparison prints its ratio diff / (gate max|want|) (run with -s).

Shapes: the fixture's coder geometries are one workgroup each (at most 49 frames, 208 samples); ``test_ops_beyond_one_workgroup`` runs
geometry 0 at 2203 samples (275 frames: two analysis workgroups of 256 frames, nine synthesis workgroups of 256 samples, a padded last
frame) against torch's fp64 convolutions with the fixture's reference kernels, which the reference's coders equal.  On the parent
commit every masked case fails with ``AttributeError: 'IstftDecoder' object has no attribute 'masked'``."""
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
TIE_MARGIN = 1e-5
LOSSES = ['si-sdr', 'log-mse', 'log1p-mse']


@pytest.fixture(scope='module')
def g18():
    d = dict(np.load(GOLDEN / 'g18_stft_tasnet.npz', allow_pickle=False))
    for k in ('cases', 'geometries', 'edges'):
        d[k] = json.loads(str(d[k]))
    spec = importlib.util.spec_from_file_location('make_golden_stft_tasnet', GOLDEN / 'make_golden_stft_tasnet.py')
    d['maker'] = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(d['maker'])             # for inputs() / coder_inputs(): the seeded signals (the reference is not imported)
    return d


def close(name, got, want, gate):
    got = got.detach().double().cpu().reshape(-1)
    want = torch.as_tensor(np.asarray(want)).double().reshape(-1)
    assert got.shape == want.shape, (name, got.shape, want.shape)
    err, bound = float((got - want).abs().max()), gate * float(want.abs().max())
    ratio = err / bound if bound > 0 else (0. if err == 0 else float('inf'))
    print(f'stft-tasnet ratio {name}: {ratio:.4f} of the gate {gate:g}')
    assert ratio <= 1.0, (name, ratio)
    return ratio


def coders(L, N, stride):
    from padertorch_amd.contrib.examples.source_separation.tasnet import IstftDecoder, StftEncoder
    return StftEncoder(L, N, stride).cuda(), IstftDecoder(L, N, stride).cuda()


# ------------------------------------------------------------------------------------------------ the three operators
@pytest.mark.parametrize('j', range(3))
def test_ops_match_the_reference_fp64(g18, j):
    geometry = g18['geometries'][j]
    L, N, stride, B, T, K = geometry
    enc, dec = coders(L, N, stride)
    p = f'k{j}_'
    x, w, mask, rx, ry, rm = (torch.from_numpy(a).cuda() for a in g18['maker'].coder_inputs(geometry, int(g18[p + 'seed'])))
    x, w, mask = x.requires_grad_(), w.requires_grad_(), mask.requires_grad_()
    e = enc(x)
    assert e.is_contiguous() and e.shape == rx.shape
    close(f'{geometry} encode', e, g18[p + 'enc'], VALUE)
    close(f'{geometry} encode dx', torch.autograd.grad((e * rx).sum(), x)[0], g18[p + 'g_x'], GRAD)
    assert torch.equal(enc(x[0]), e[0])                                          # [T] -> [N, E]
    y = dec(w)
    close(f'{geometry} decode', y, g18[p + 'dec'], VALUE)
    close(f'{geometry} decode dw', torch.autograd.grad((y * ry).sum(), w)[0], g18[p + 'g_w'], GRAD)
    my = dec.masked(mask, w)
    assert my.shape == rm.shape
    close(f'{geometry} masked decode', my, g18[p + 'mdec'], VALUE)
    gm, ge = torch.autograd.grad((my * rm).sum(), [mask, w])
    close(f'{geometry} masked decode dmask', gm, g18[p + 'g_mask'], GRAD)
    close(f'{geometry} masked decode dencoded', ge, g18[p + 'g_enc'], GRAD)


def test_frame_count_edges(g18):
    enc, dec = coders(16, 64, None)
    for T in g18['edges']:                                                       # 16 and 15 samples: one frame; 17: two
        x = torch.from_numpy(g18[f'e{T}_x']).float().cuda().requires_grad_()
        e = enc(x)
        assert e.shape == g18[f'e{T}_enc'].shape
        close(f'{T} samples encode', e, g18[f'e{T}_enc'], VALUE)
        y = dec(e)
        close(f'{T} samples decode', y, g18[f'e{T}_dec'], VALUE)
        gx = torch.autograd.grad(y.sum(), x)[0]
        assert gx.shape == x.shape and bool(torch.isfinite(gx).all())


def test_ops_beyond_one_workgroup(g18):
    from padertorch_amd import ops
    L, N, hop, B, T, K = 16, 64, 8, 2, 2203, 2
    enc, dec = coders(L, N, None)
    E = ops.stft_coders.stft_frames(T, L, hop)
    Tp = (E - 1) * hop + L
    assert (E, Tp) == (275, 2208)
    k_a = torch.from_numpy(g18['k0_stft_kernel'])
    k_re, k_im = torch.from_numpy(g18['k0_istft_kernel_real']), torch.from_numpy(g18['k0_istft_kernel_imag'])

    def decode64(w):
        """The reference's inverse (``_stft.py:226-255``) on ``[B, N, E]`` fp64."""
        re, im = w[:, :N // 2], w[:, N // 2:]
        re, im = torch.cat([re, re[:, 1:-1].flip(1)], 1), torch.cat([im, -im[:, 1:-1].flip(1)], 1)
        return (F.conv_transpose1d(re, k_re, stride=hop) + F.conv_transpose1d(im, k_im, stride=hop))[:, 0]

    gen = torch.Generator().manual_seed(181)
    x0, m0 = torch.randn(B, T, generator=gen), torch.rand(K, B, N, E, generator=gen)
    rx, rm = torch.randn(B, N, E, generator=gen), torch.randn(K, B, Tp, generator=gen)
    x64, m64 = x0.double().requires_grad_(), m0.double().requires_grad_()
    e64 = F.conv1d(F.pad(x64, (0, Tp - T))[:, None], k_a, stride=hop)
    my64 = torch.stack([decode64(m64[k] * e64) for k in range(K)])
    want = torch.autograd.grad((e64 * rx.double()).sum() + (my64 * rm.double()).sum(), [x64, m64])
    x, m = x0.cuda().requires_grad_(), m0.cuda().requires_grad_()
    e = enc(x)
    my = dec.masked(m, e)
    got = torch.autograd.grad((e * rx.cuda()).sum() + (my * rm.cuda()).sum(), [x, m])
    close('275 frames encode', e, e64.detach(), VALUE)
    close('275 frames masked decode', my, my64.detach(), VALUE)
    close('275 frames dx', got[0], want[0], GRAD)
    close('275 frames dmask', got[1], want[1], GRAD)


def test_masked_decode_is_the_decode_of_the_product_and_repeats(g18):
    geometry = g18['geometries'][1]
    L, N, stride, B, T, K = geometry
    _, dec = coders(L, N, stride)
    _, w, mask, _, _, rm = (torch.from_numpy(a).cuda() for a in g18['maker'].coder_inputs(geometry, int(g18['k1_seed'])))
    w, mask = w.requires_grad_(), mask.requires_grad_()
    first = dec.masked(mask, w)
    second = dec.masked(mask, w)
    assert torch.equal(first, second)
    g1 = torch.autograd.grad((first * rm).sum(), [mask, w])
    g2 = torch.autograd.grad((second * rm).sum(), [mask, w])
    assert all(torch.equal(a, b) for a, b in zip(g1, g2))
    product = torch.stack([dec(mask[k] * w) for k in range(K)])
    close('masked decode against the decode of the product', first, product.detach().double().cpu(), VALUE)
    g3 = torch.autograd.grad((product * rm).sum(), [mask, w])
    for name, a, b in zip(('dmask', 'dencoded'), g1, g3):
        close(f'masked decode {name} against the product\'s', a, b.double().cpu(), GRAD)
    only = torch.autograd.grad((dec.masked(mask, w.detach()) * rm).sum(), mask)[0]           # encoded without a gradient
    assert torch.equal(only, g1[0])


def test_other_dtypes_are_refused():
    enc, dec = coders(16, 64, None)
    with pytest.raises(NotImplementedError, match='float32 only'):
        enc(torch.zeros(2, 100, device='cuda', dtype=torch.float64))
    with pytest.raises(NotImplementedError, match='float32 only'):
        dec.masked(torch.zeros(2, 2, 64, 5, device='cuda'), torch.zeros(2, 64, 5, device='cuda', dtype=torch.float16))


# ------------------------------------------------------------------------------------------------ the whole model
def build_model(g18, index):
    from padertorch_amd.contrib.examples.source_separation.tasnet import IstftDecoder, StftEncoder, TasNet
    from padertorch_amd.modules import DPRNN, ConvNet
    c = g18['cases'][index]
    if c['kind'] == 'dprnn':
        separator = DPRNN(c['sep_in'], c['rnn_size'], c['window'], c['hop'], c['blocks'])
    else:
        separator = ConvNet(input_size=c['sep_in'], num_blocks=c['blocks'], num_repeats=c['repeats'], hidden_channels=c['hidden'],
                            kernel_size=3, norm=c['norm'])
    net = TasNet(StftEncoder(c['L'], c['N'], c['stride']), separator, IstftDecoder(c['L'], c['N'], c['stride']), mask=c['mask'],
                 output_nonlinearity=c['nonlinearity'], num_speakers=c['K'], additional_out_size=c['A'])
    p = f'c{index}_'
    net.load_state_dict({k: torch.from_numpy(g18[p + 'p_' + k]) for k in json.loads(str(g18[p + 'keys']))}, strict=True)
    return net.cuda(), c, p


@pytest.mark.parametrize('index', range(4))
def test_model_matches_the_reference_fp64(g18, index):
    net, c, p = build_model(g18, index)
    assert float(g18[p + 'margin']) >= TIE_MARGIN                         # a condition on the inputs: no sign decision near a tie
    names = json.loads(str(g18[p + 'names']))
    params = dict(net.named_parameters())
    assert list(params) == names
    y0, s0, r0, r20 = (torch.from_numpy(a).cuda() for a in g18['maker'].inputs(c, int(g18[p + 'seed'])))
    y = y0.requires_grad_()
    batch = dict(y=list(y.unbind(0)), s=s0, num_samples=list(c['num_samples']))
    out = net(batch)
    B, K, T, A, E = c['B'], c['K'], c['T'], c['A'], g18['maker'].frames(c)
    assert out['out'].shape == (B, K, T) and out['encoded'].shape == (B, E, c['N'])
    assert [int(n) for n in out['encoded_sequence_lengths']] == [int(n) for n in g18[p + 'lengths']]
    close(f'case {index} out', out['out'], g18[p + 'out64'], VALUE)
    functional = (out['out'] * r0).sum()
    if A:
        assert out['additional_out'].shape == (B, A, E)
        close(f'case {index} additional_out', out['additional_out'], g18[p + 'add64'], VALUE)
        functional = functional + (out['additional_out'] * r20).sum()
    losses = net.loss(batch, out)
    close(f'case {index} losses', torch.stack([losses[k] for k in LOSSES]), g18[p + 'loss64'], VALUE)
    leaves = [params[n] for n in names] + [y]
    if c['kind'] == 'dprnn':                     # the chunk LSTM's backward runs once per forward: a second forward for the second gradient
        gf = torch.autograd.grad(functional, leaves)
        losses = net.loss(batch, net(batch))
    else:
        gf = torch.autograd.grad(functional, leaves, retain_graph=True)
    gl = torch.autograd.grad(losses['si-sdr'], leaves)
    worst_f = max(close(f'case {index} functional d {n}', g, g18[p + 'gf64_' + n], GRAD) for n, g in zip(names + ['y'], gf))
    worst_l = max(close(f'case {index} si-sdr d {n}', g, g18[p + 'gl64_' + n], GRAD) for n, g in zip(names + ['y'], gl))
    print(f'stft-tasnet ratio case {index} worst gradient: functional {worst_f:.4f}, si-sdr {worst_l:.4f}')


def _step(net, y, r, lengths):
    """forward + backward of sum(out r): [out, d y, d parameters...]."""
    y = y.detach().requires_grad_()
    out = net(dict(y=y, num_samples=lengths))['out']
    grads = torch.autograd.grad((out * r).sum(), [y] + list(net.parameters()))
    return [out.detach()] + list(grads)


def test_encoder_returns_device_lengths_without_a_synchronisation(g18):
    enc, _ = coders(16, 64, None)
    y = torch.randn(3, 203, device='cuda')
    lengths = torch.tensor([203, 150, 97], device='cuda')
    enc(y, lengths)                                                              # warm-up: library load, allocator
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('error')
    try:
        encoded, frames = enc(y, lengths)
    finally:
        torch.cuda.set_sync_debug_mode('default')
    assert frames.is_cuda and frames.dtype == torch.int64 and frames.tolist() == g18['c0_lengths'].tolist()
    assert encoded.shape == (3, 64, 25)
    host = enc(y, [203, 150, 97])[1]
    assert not host.is_cuda and host.dtype == torch.int64 and host.tolist() == frames.tolist()


def test_runs_are_bit_identical_and_capturable(g18):
    from padertorch_amd.ops import capture
    net, c, p = build_model(g18, 0)
    y, _, r, _ = (torch.from_numpy(a).cuda() for a in g18['maker'].inputs(c, int(g18[p + 'seed'])))
    lengths = torch.tensor(c['num_samples'], device='cuda')
    first, second = _step(net, y, r, lengths), _step(net, y, r, lengths)
    for i, (a, b) in enumerate(zip(first, second)):
        assert torch.equal(a, b), i
    sy, sr, sl = y.clone(), r.clone(), lengths.clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        _step(net, sy, sr, sl)                                         # eager warm-up on the capture stream
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with capture.capture_mode():
        with torch.cuda.graph(graph, stream=side):
            capture.zero_block(sy.device)
            captured = _step(net, sy, sr, sl)
    graph.replay()
    torch.cuda.synchronize()
    for i, (a, b) in enumerate(zip(captured, first)):
        assert torch.equal(a, b), ('replay', i)
    other = torch.tensor([120, 203, 16], device='cuda')                   # another pattern: the lengths are device data
    sl.copy_(other)
    graph.replay()
    torch.cuda.synchronize()
    eager = _step(net, y, r, other)
    assert not torch.equal(eager[0], first[0])
    for i, (a, b) in enumerate(zip(captured, eager)):
        assert torch.equal(a, b), ('replay with other lengths', i)


def test_or_pit_over_an_stft_tasnet():
    from padertorch_amd.contrib.examples.source_separation.or_pit import OneAndRestPIT
    from padertorch_amd.contrib.examples.source_separation.tasnet import IstftDecoder, StftEncoder, TasNet
    from padertorch_amd.modules import ConvNet
    torch.manual_seed(182)
    separator = TasNet(StftEncoder(16, 64), ConvNet(input_size=8, num_blocks=2, num_repeats=1, hidden_channels=16, kernel_size=3),
                       IstftDecoder(16, 64), num_speakers=2, additional_out_size=5)
    net = OneAndRestPIT(separator, flag_units=5).cuda()
    B, K, T = 2, 3, 203
    batch = dict(y=torch.randn(B, T, device='cuda'), s=torch.randn(B, K, T, device='cuda'), num_samples=[T] * B, num_speakers=[K] * B)
    out = net(batch)
    loss = net.loss(batch, out)['loss']
    grads = torch.autograd.grad(loss, list(net.parameters()))
    assert bool(torch.isfinite(loss)) and out['out'].shape[0] == B and out['out'].shape[-1] == T
    assert all(bool(torch.isfinite(g).all()) for g in grads) and any(float(g.abs().max()) > 0 for g in grads)
