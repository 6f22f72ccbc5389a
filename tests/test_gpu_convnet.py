"""ConvNet (the Conv-TasNet separator) and its kernels (csrc/tcn.hip) against the reference's fp64 results
(tests/golden/g14_convnet.npz) and fp64 restatements with torch's own operators on the CPU.

Gates (the project's own, tests/test_gpu_td.py / test_gpu_tas_coders.py): values |diff| <= 1e-5 max|want|, gradients |diff| <= 2e-4 max|want|.
The reference's own fp32 run differs from its fp64 run by at most 2.3e-7 max|want| in the output, 1.9e-7 in dx and 5.8e-5 in the worst
parameter gradient (a PReLU slope of the 3x2 gLN case) on the fixture.  Every comparison prints its ratio diff / (gate max|want|)
(run with -s; profiles/convnet.txt).

The operator tests draw u, bias (multiples of 1/8), taps (multiples of 1/4) and slopes (0.25, 0.5) from a dyadic grid, magnitudes at most 4:
every pre-activation is then exact in fp32 in any summation order, so the sign decisions of both PReLUs agree with fp64 by construction,
zeros included."""
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
def g14():
    d = dict(np.load(GOLDEN / 'g14_convnet.npz', allow_pickle=False))
    d['cases'] = json.loads(str(d['cases']))
    spec = importlib.util.spec_from_file_location('make_golden_convnet', GOLDEN / 'make_golden_convnet.py')
    d['maker'] = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(d['maker'])             # for inputs(): the seeded x and r (the reference is not imported)
    return d


def close(name, got, want, gate):
    got = got.detach().double().cpu().reshape(-1)
    want = torch.as_tensor(np.asarray(want)).double().reshape(-1)
    assert got.shape == want.shape, (name, got.shape, want.shape)
    ratio = float((got - want).abs().max() / (gate * want.abs().max()))
    print(f'convnet ratio {name}: {ratio:.4f} of the gate {gate:g}')
    assert ratio <= 1.0, (name, ratio)
    return ratio


def non_contiguous(x):
    """The same values behind a stride of two along the channel axis."""
    wide = torch.zeros(x.shape[0], x.shape[1], 2 * x.shape[2] + 1, device=x.device)
    wide[:, :, 1::2] = x
    view = wide[:, :, 1::2]
    assert not view.is_contiguous() and torch.equal(view, x)
    return view


@pytest.mark.parametrize('index', range(4))
def test_network_matches_the_reference_fp64(g14, index):
    from padertorch_amd.modules import ConvNet
    case = g14['cases'][index]
    N, H, K, blocks, repeats, norm, B, T = case
    p = f'c{index}_'
    net = ConvNet(input_size=N, num_blocks=blocks, num_repeats=repeats, hidden_channels=H, kernel_size=K, norm=norm)
    net.load_state_dict({k: torch.from_numpy(g14[p + 'p_' + k]) for k in json.loads(str(g14[p + 'keys']))}, strict=True)
    net.cuda()
    x, r = (torch.from_numpy(a).cuda() for a in g14['maker'].inputs(case, int(g14[p + 'seed'])))
    x = non_contiguous(x).requires_grad_()
    y = net(x, torch.tensor([T] * B))
    assert y.shape == (B, T, N)
    names = json.loads(str(g14[p + 'names']))
    params = dict(net.named_parameters())
    assert list(params) == names
    grads = torch.autograd.grad((y * r).sum(), [x] + [params[n] for n in names])
    close(f'{case} y', y, g14[p + 'y64'], VALUE)
    close(f'{case} dx', grads[0], g14[p + 'g64_x'], GRAD)
    worst = max(close(f'{case} d {n}', g, g14[p + 'g64_' + n], GRAD) for n, g in zip(names, grads[1:]))
    print(f'convnet ratio {case} worst parameter gradient: {worst:.4f}')


def dyadic(gen, shape, step, limit=4):
    n = int(limit / step)
    return torch.randint(-n, n + 1, shape, generator=gen).float() * step


def depthwise_fp64(u, a1, w, b, a2, d, K):
    """prelu -> pad -> depthwise conv -> prelu with torch's operators on [B, H, T], and the per-example statistics of the result."""
    from padertorch_amd.ops.tcn import depthwise_pad
    z = F.conv1d(F.pad(F.prelu(u.transpose(1, 2), a1), depthwise_pad(K, d)), w, b, dilation=d, groups=u.shape[2])
    v = F.prelu(z, a2).transpose(1, 2)
    mean = v.mean((1, 2))
    return v, mean, 1 / torch.sqrt(((v - mean[:, None, None]) ** 2).mean((1, 2)) + 1e-5)


#: (B, T, H, K, d): more than one time tile (64 rows) and channel block, a halo of 128 rows on either side (the reference's largest
#: dilation) against tiles of 64; an even kernel with odd channels (scalar loads); K = 1 over two channel blocks of the scalar path
DEPTHWISE = [(2, 301, 128, 3, 1), (2, 301, 128, 3, 128), (1, 70, 7, 4, 2), (3, 5, 257, 1, 1)]


@pytest.mark.parametrize('cfg', DEPTHWISE, ids=lambda c: 'x'.join(map(str, c)))
def test_depthwise_prelu_against_fp64(cfg):
    from padertorch_amd import ops
    B, T, H, K, d = cfg
    gen = torch.Generator().manual_seed(41)
    host = [dyadic(gen, (B, T, H), 1 / 8), torch.tensor([0.25]), dyadic(gen, (H, 1, K), 1 / 4), dyadic(gen, (H,), 1 / 8), torch.tensor([0.5])]
    gv = torch.randn(B, T, H, generator=gen)
    ref = [t.double().requires_grad_() for t in host]
    want_v, want_mean, want_rstd = depthwise_fp64(*ref, d, K)
    want = torch.autograd.grad((want_v * gv.double()).sum(), ref)
    dev = [t.cuda().requires_grad_() for t in host]
    v, stats = ops.depthwise_prelu(*dev, d, K)
    assert not stats.requires_grad and stats.shape == (B, 2)
    got = torch.autograd.grad((v * gv.cuda()).sum(), dev)
    close(f'{cfg} v', v, want_v.detach(), VALUE)
    assert torch.equal(v.cpu().double(), want_v.detach())               # exact by construction
    close(f'{cfg} mean', stats[:, 0], want_mean.detach(), VALUE)
    close(f'{cfg} rstd', stats[:, 1], want_rstd.detach(), VALUE)
    for name, g, w in zip(('gu', 'd slope_in', 'd weight', 'd bias', 'd slope_out'), got, want):
        close(f'{cfg} {name}', g, w, GRAD)
    # the statistics the fused launch leaves behind are those of channel_norm's own statistics pass on v
    own = torch.ops.ptmi.tcn_norm_stats(v.detach(), False, 1e-5)
    close(f'{cfg} fused mean vs statistics pass', stats[:, 0], own[:, 0].double().cpu(), VALUE)
    close(f'{cfg} fused rstd vs statistics pass', stats[:, 1], own[:, 1].double().cpu(), VALUE)
    # and the norm that takes them skips that pass without changing its result
    gamma, beta = torch.rand(H, 1, generator=gen).cuda() + 0.5, torch.rand(H, 1, generator=gen).cuda() - 0.5
    close(f'{cfg} norm with fused statistics', ops.channel_norm(v.detach(), gamma, beta, 'example', stats=stats),
          ops.channel_norm(v.detach(), gamma, beta, 'example').double().cpu(), VALUE)


def norm_fp64(x, gamma, beta, groups):
    dims = (1, 2) if groups == 'example' else (2,)
    mean = x.mean(dims, keepdim=True)
    var = ((x - mean) ** 2).mean(dims, keepdim=True)
    return gamma.reshape(-1) * (x - mean) / torch.sqrt(var + 1e-5) + beta.reshape(-1)


@pytest.mark.parametrize('groups', ['example', 'row'])
@pytest.mark.parametrize('shape', [(2, 301, 128), (3, 5, 257)], ids=lambda s: 'x'.join(map(str, s)))
def test_channel_norm_against_fp64(shape, groups):
    from padertorch_amd import ops
    gen = torch.Generator().manual_seed(43)
    C = shape[2]
    pshape = (C, 1) if groups == 'example' else (C,)
    host = [torch.randn(shape, generator=gen) * 2 + 0.7, torch.rand(pshape, generator=gen) + 0.5, torch.rand(pshape, generator=gen) - 0.5]
    gy = torch.randn(shape, generator=gen)
    ref = [t.double().requires_grad_() for t in host]
    want_y = norm_fp64(*ref, groups)
    want = torch.autograd.grad((want_y * gy.double()).sum(), ref)
    dev = [t.cuda().requires_grad_() for t in host]
    y = ops.channel_norm(*dev, groups)
    got = torch.autograd.grad((y * gy.cuda()).sum(), dev)
    close(f'{shape} {groups} y', y, want_y.detach(), VALUE)
    for name, g, w in zip(('dx', 'd gamma', 'd beta'), got, want):
        assert g.shape == w.shape
        close(f'{shape} {groups} {name}', g, w, GRAD)


def _block_pass(block, x, r):
    x = x.detach().requires_grad_()
    y = block(x)
    grads = torch.autograd.grad((y * r).sum(), [x] + list(block.parameters()))
    return [y.detach()] + list(grads)


def _block_inputs(seed, B=2, T=150, N=24):
    gen = torch.Generator().manual_seed(seed)
    return torch.randn(B, T, N, generator=gen).cuda(), torch.randn(B, T, N, generator=gen).cuda()


def test_runs_are_bit_identical_and_capturable():
    from padertorch_amd.modules.convnet import _Conv1DBlock
    from padertorch_amd.ops import capture
    torch.manual_seed(5)
    block = _Conv1DBlock(24, 40, 3, dilation=2, norm='gLN').cuda()
    x, r = _block_inputs(51)
    first, second = _block_pass(block, x, r), _block_pass(block, x, r)
    for a, b in zip(first, second):
        assert torch.equal(a, b)
    sx, sr = x.clone(), r.clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        _block_pass(block, sx, sr)                                # eager warm-up on the capture stream
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with capture.capture_mode():                                  # (the dense layers' zeroed words come from nodes of the graph)
        with torch.cuda.graph(graph, stream=side):
            capture.zero_block(sx.device)
            captured = _block_pass(block, sx, sr)
    for seed in (52, 53):
        x, r = _block_inputs(seed)
        sx.copy_(x), sr.copy_(r)
        graph.replay()
        torch.cuda.synchronize()
        eager = _block_pass(block, x, r)
        for i, (a, b) in enumerate(zip(captured, eager)):
            assert torch.equal(a, b), (seed, i)


def test_other_dtypes_are_refused():
    from padertorch_amd import ops
    from padertorch_amd.modules import ConvNet
    with pytest.raises(NotImplementedError, match='float32'):
        ConvNet(8, 1, 1, 16, 3).cuda()(torch.zeros(1, 9, 8, device='cuda', dtype=torch.float64))
    with pytest.raises(NotImplementedError, match='float32'):
        ops.channel_norm(torch.zeros(1, 9, 8, device='cuda', dtype=torch.float16), torch.ones(8, device='cuda'), torch.zeros(8, device='cuda'))
