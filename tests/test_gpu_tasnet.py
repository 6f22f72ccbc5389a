"""TasNet (encoder to loss) and its glue kernels (csrc/tasnet.hip) against the reference's fp64 results (tests/golden/g15_tasnet.npz) and
fp64 restatements with torch's own operators on the CPU.

Gates (the project's own, tests/test_gpu_convnet.py): values |diff| <= 1e-5 max|want|, gradients |diff| <= 2e-4 max|want|.  On the fixture
the reference's own fp32 run differs from its fp64 run by at most these shares OF A GATE (tests/golden/make_golden_tasnet.py prints them
and refuses a seed above one half): out 0.024, additional_out 0.020, the three losses 0.014, the gradients of the functional
sum(out r) + sum(additional_out r2) 0.011, the gradients of the si-sdr loss 0.030.  Every comparison prints its ratio
diff / (gate max|want|) (run with -s).

Shapes chosen by reading csrc/tasnet.hip (tiles of 32 frames; 256 channels per tile in the entry norm's forward, 128 in its backward, 64
in the mask head; 8192 elements per PReLU workgroup; 2048 samples per centring workgroup, 256 partials per finalize trip):
  entry norm   (2, 256, 70): one channel block forward, two backward, three frame tiles with a tail of 6; (1, 5, 65): scalar on both sides,
               one frame past two tiles; (3, 64, 1): one frame, vector on the channels-last side only; (2, 260, 64): the two-stage row sum
               forward (two blocks) and backward (three), exactly two tiles, vector on both sides; lengths None / full / partial with one
               example of length 0 (and one dead whole tile), int32 and int64
  mask head    (B, E, N, K, A) = (2, 70, 256, 2, 0): eight channel blocks, vector channels-last side, scalar channels-first side;
               (2, 65, 5, 3, 3): C = 18 in one block with the additional rows, scalar; (1, 64, 6, 2, 4): vector on both sides with A
               inside the first quad row range; all six activations; g_additional None
  centre       T' = T, T' > T (the crop, and the zeros of the backward), T' < T, T = 1, lengths that are multiples of 4 (vector) and not;
               526340 samples: 258 partials, a second trip of the finalize loop
  PReLU        C = 256 (five workgroups, vector) and 3 x 65 x 7 elements (odd: scalar); dyadic inputs with exact zeros
  alignment    contiguous views one float into their storage pick the scalar kernels on that side: elementwise results equal the vector
               kernels' bit for bit, the sentinels around the views stay
Inputs whose sign decides something (PReLU, relu, leaky_relu, elu) come from a dyadic grid: exact in fp32, zeros included."""
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
def g15():
    d = dict(np.load(GOLDEN / 'g15_tasnet.npz', allow_pickle=False))
    d['cases'] = json.loads(str(d['cases']))
    spec = importlib.util.spec_from_file_location('make_golden_tasnet', GOLDEN / 'make_golden_tasnet.py')
    d['maker'] = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(d['maker'])             # for inputs(): the seeded signals (the reference is not imported)
    return d


def close(name, got, want, gate):
    got = got.detach().double().cpu().reshape(-1)
    want = torch.as_tensor(np.asarray(want)).double().reshape(-1)
    assert got.shape == want.shape, (name, got.shape, want.shape)
    err, bound = float((got - want).abs().max()), gate * float(want.abs().max())
    ratio = err / bound if bound > 0 else (0. if err == 0 else float('inf'))      # want == 0 everywhere: the bound is zero
    print(f'tasnet ratio {name}: {ratio:.4f} of the gate {gate:g}')
    assert ratio <= 1.0, (name, ratio)
    return ratio


def _id(cfg):
    return 'x'.join(map(str, cfg))


def dyadic(gen, shape, step, limit=4):
    n = int(limit / step)
    return torch.randint(-n, n + 1, shape, generator=gen).float() * step


# ------------------------------------------------------------------------------------------------ the whole model
def build_model(g15, index):
    from padertorch_amd.contrib.examples.source_separation.tasnet import TasDecoder, TasEncoder, TasNet
    from padertorch_amd.modules import ConvNet
    c = g15['cases'][index]
    net = TasNet(TasEncoder(c['L'], c['n_enc'], c['stride']),
                 ConvNet(input_size=c['sep_in'], num_blocks=c['blocks'], num_repeats=c['repeats'], hidden_channels=c['hidden'], kernel_size=3,
                         norm=c['norm']),
                 TasDecoder(c['L'], c['n_dec'], c['stride']), mask=c['mask'], output_nonlinearity=c['nonlinearity'], num_speakers=c['K'],
                 additional_out_size=c['A'])
    p = f'c{index}_'
    net.load_state_dict({k: torch.from_numpy(g15[p + 'p_' + k]) for k in json.loads(str(g15[p + 'keys']))}, strict=True)
    return net.cuda(), c, p


@pytest.mark.parametrize('index', range(4))
def test_model_matches_the_reference_fp64(g15, index):
    net, c, p = build_model(g15, index)
    assert float(g15[p + 'margin']) >= TIE_MARGIN                         # a condition on the inputs: no sign decision near a tie
    names = json.loads(str(g15[p + 'names']))
    params = dict(net.named_parameters())
    assert list(params) == names
    y0, s0, r0, r20 = (torch.from_numpy(a).cuda() for a in g15['maker'].inputs(c, int(g15[p + 'seed'])))
    y = y0.requires_grad_()
    batch = dict(y=list(y.unbind(0)), s=s0, num_samples=list(c['num_samples']))
    out = net(batch)
    B, K, T, A, E = c['B'], c['K'], c['T'], c['A'], g15['maker'].frames(c)
    assert out['out'].shape == (B, K, T) and out['encoded'].shape == (B, E, c['n_enc']) and 'encoded_out' not in out
    assert [int(n) for n in out['encoded_sequence_lengths']] == [int(n) for n in g15[p + 'lengths']]
    close(f'case {index} out', out['out'], g15[p + 'out64'], VALUE)
    functional = (out['out'] * r0).sum()
    if A:
        assert out['additional_out'].shape == (B, A, E)
        close(f'case {index} additional_out', out['additional_out'], g15[p + 'add64'], VALUE)
        functional = functional + (out['additional_out'] * r20).sum()
    else:
        assert 'additional_out' not in out
    review = net.review(batch, out)
    assert list(review['losses']) == LOSSES and set(review['audios']) == {'observation'} | {f'{k}/{i}' for k in ('estimate', 'target')
                                                                                          for i in range(K)}
    close(f'case {index} losses', torch.stack([review['losses'][k] for k in LOSSES]), g15[p + 'loss64'], VALUE)
    leaves = [params[n] for n in names] + [y]
    gf = torch.autograd.grad(functional, leaves, retain_graph=True)
    gl = torch.autograd.grad(review['losses']['si-sdr'], leaves)
    worst_f = max(close(f'case {index} functional d {n}', g, g15[p + 'gf64_' + n], GRAD) for n, g in zip(names + ['y'], gf))
    worst_l = max(close(f'case {index} si-sdr d {n}', g, g15[p + 'gl64_' + n], GRAD) for n, g in zip(names + ['y'], gl))
    print(f'tasnet ratio case {index} worst gradient: functional {worst_f:.4f}, si-sdr {worst_l:.4f}')


def test_encoded_out_on_request(g15):
    net, c, p = build_model(g15, 0)
    y0, s0, _, _ = (torch.from_numpy(a).cuda() for a in g15['maker'].inputs(c, int(g15[p + 'seed'])))
    batch = dict(y=y0, s=s0, num_samples=torch.tensor(c['num_samples']))
    plain = net(batch)
    net.return_encoded_out = True
    out = net(batch)
    assert torch.equal(out['out'], plain['out'])
    assert out['encoded_out'].shape == (c['B'], c['K'], g15['maker'].frames(c), c['n_enc'])
    # out = centre(decode(mask * encoded)): decode encoded_out with the plain decoder and compare
    from padertorch_amd.ops import tasnet as glue
    est = out['encoded_out'].permute(1, 0, 3, 2).reshape(c['K'] * c['B'], c['n_enc'], -1)
    again = glue.center(net.decoder(est).view(c['K'], c['B'], -1), c['T'])
    close('encoded_out decoded again', again, out['out'].detach().double().cpu(), VALUE)
    assert out['encoded_out'].requires_grad


def _step(net, y, r, lengths):
    """forward + backward of sum(out r): [out, d y, d parameters...].  (The loss is left out of the captured step: ``pit_from_stats``
    builds its permutation table from a host list on every call, which a capture does not permit.)"""
    y = y.detach().requires_grad_()
    out = net(dict(y=y, num_samples=lengths))['out']
    grads = torch.autograd.grad((out * r).sum(), [y] + list(net.parameters()))
    return [out.detach()] + list(grads)


def test_runs_are_bit_identical_and_capturable(g15):
    from padertorch_amd.ops import capture
    net, c, p = build_model(g15, 0)
    y, _, r, _ = (torch.from_numpy(a).cuda() for a in g15['maker'].inputs(c, int(g15[p + 'seed'])))
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


def test_nan_stays_in_its_example(g15):
    net, c, p = build_model(g15, 0)
    y, s, _, _ = (torch.from_numpy(a).cuda() for a in g15['maker'].inputs(c, int(g15[p + 'seed'])))
    clean = net(dict(y=y, s=s, num_samples=c['num_samples']))['out']
    y[1, 40] = float('nan')
    out = net(dict(y=y, s=s, num_samples=c['num_samples']))['out']
    assert bool(torch.isnan(out[1]).any())
    assert bool(torch.isfinite(out[0]).all()) and bool(torch.isfinite(out[2]).all())
    # (finite, not unchanged: the dense layers scale their operands by one absolute maximum over all rows, which the NaN moves)
    assert clean.shape == out.shape and bool(torch.isfinite(clean).all())


def test_other_dtypes_are_refused():
    from padertorch_amd.ops import tasnet as glue
    z = torch.zeros(1, 4, 8, device='cuda', dtype=torch.float64)
    with pytest.raises(NotImplementedError, match='float32'):
        glue.mask_head(z, 2, 4)
    with pytest.raises(NotImplementedError, match='float32'):
        glue.prelu_rows(z.half(), torch.ones(1, device='cuda'))
    with pytest.raises(NotImplementedError, match='float32'):
        glue.center(z, 8)
    with pytest.raises(NotImplementedError, match='float32'):
        glue.entry_norm(z, torch.ones(4, device='cuda'), torch.zeros(4, device='cuda'))


# ------------------------------------------------------------------------------------------------ entry norm
def entry_norm_fp64(w, gamma, beta, lengths, eps=1e-5):
    y = F.layer_norm(w.transpose(1, 2), (w.shape[1],), gamma, beta, eps)
    if lengths is None:
        return y
    live = torch.arange(w.shape[2])[None, :] < torch.as_tensor(lengths)[:, None]
    return y * live[:, :, None].to(y.dtype)


def _lengths_of(mode, B, E):
    if mode == 'none':
        return None
    if mode == 'full':
        return torch.full((B,), E, dtype=torch.int64)
    values = [max(E - 37, (E + 1) // 2), 0, E][:B] if B > 1 else [(E + 1) // 2]      # B = 2, E = 70: 35 frames: a dead whole tile
    return torch.tensor(values, dtype=torch.int32 if mode == 'partial32' else torch.int64)


@pytest.mark.parametrize('mode', ['none', 'full', 'partial32', 'partial64'])
@pytest.mark.parametrize('shape', [(2, 256, 70), (1, 5, 65), (3, 64, 1), (2, 260, 64), (2, 37, 201)], ids=_id)
def test_entry_norm_against_fp64(shape, mode):
    """(2, 37, 201): 14 partials (B x tiles of 32 frames) of width 2 N = 74 through colreduce_kernel (csrc/reduce.h): every one of its four
    chains adds more than one partial, and its second column block ends inside the block."""
    from padertorch_amd.ops import tasnet as glue
    B, N, E = shape
    gen = torch.Generator().manual_seed(151)
    host = [torch.randn(shape, generator=gen) * 2 + 0.7, torch.rand(N, generator=gen) + 0.5, torch.rand(N, generator=gen) - 0.5]
    gy = torch.randn(B, E, N, generator=gen)
    lengths = _lengths_of(mode, B, E)
    ref = [t.double().requires_grad_() for t in host]
    want_y = entry_norm_fp64(*ref, lengths)
    want = torch.autograd.grad((want_y * gy.double()).sum(), ref)
    dev = [t.cuda().requires_grad_() for t in host]
    y = glue.entry_norm(*dev, None if lengths is None else lengths.cuda())
    got = torch.autograd.grad((y * gy.cuda()).sum(), dev)
    assert y.shape == (B, E, N) and y.is_contiguous()
    close(f'{shape} {mode} y', y, want_y.detach(), VALUE)
    if lengths is not None:
        dead = (torch.arange(E)[None, :] >= lengths[:, None])
        assert bool((y.cpu()[dead] == 0).all()) and bool((got[0].cpu().transpose(1, 2)[dead] == 0).all())     # zero, not beta
    for name, g, w in zip(('dw', 'd gamma', 'd beta'), got, want):
        assert g.shape == w.shape
        close(f'{shape} {mode} {name}', g, w, GRAD)
    if mode == 'partial64':                                              # a list and a CPU tensor are the same lengths
        assert torch.equal(glue.entry_norm(*dev, [int(n) for n in lengths]), y) and torch.equal(glue.entry_norm(*dev, lengths), y)


# ------------------------------------------------------------------------------------------------ PReLU
@pytest.mark.parametrize('shape', [(2, 70, 256), (3, 65, 7)], ids=_id)
def test_prelu_rows_against_fp64(shape):
    from padertorch_amd.ops import tasnet as glue
    gen = torch.Generator().manual_seed(152)
    host = [dyadic(gen, shape, 1 / 8), torch.tensor([0.25])]
    assert int((host[0] == 0).sum()) > 0
    g = torch.randn(shape, generator=gen)
    ref = [t.double().requires_grad_() for t in host]
    want_y = F.prelu(*ref)
    want = torch.autograd.grad((want_y * g.double()).sum(), ref)
    dev = [t.cuda().requires_grad_() for t in host]
    y = glue.prelu_rows(*dev)
    got = torch.autograd.grad((y * g.cuda()).sum(), dev)
    assert torch.equal(y.cpu().double(), want_y.detach())               # exact by construction
    close(f'{shape} prelu gx', got[0], want[0], GRAD)
    close(f'{shape} prelu d slope', got[1], want[1], GRAD)
    only = [host[0].cuda().requires_grad_(), host[1].cuda()]
    (glue.prelu_rows(*only) * g.cuda()).sum().backward()
    assert torch.equal(only[0].grad, got[0]) and only[1].grad is None


# ------------------------------------------------------------------------------------------------ mask head
ACTS = {'sigmoid': torch.sigmoid, 'relu': F.relu, 'leaky_relu': F.leaky_relu, 'elu': F.elu, 'tanh': torch.tanh, 'identity': lambda z: z}


def head_fp64(z, K, N, A, activation):
    B, E, _ = z.shape
    m = ACTS[activation](z[..., A:]).reshape(B, E, K, N).permute(2, 0, 3, 1)
    return m, z[..., :A].transpose(1, 2)


@pytest.mark.parametrize('activation', list(ACTS))
@pytest.mark.parametrize('cfg', [(2, 70, 256, 2, 0), (2, 65, 5, 3, 3), (1, 64, 6, 2, 4)], ids=_id)
def test_mask_head_against_fp64(cfg, activation):
    from padertorch_amd.ops import tasnet as glue
    B, E, N, K, A = cfg
    gen = torch.Generator().manual_seed(153)
    z0 = dyadic(gen, (B, E, A + K * N), 1 / 8)
    gm, ga = torch.randn(K, B, N, E, generator=gen), torch.randn(B, A, E, generator=gen)
    ref = z0.double().requires_grad_()
    want_m, want_a = head_fp64(ref, K, N, A, activation)
    z = z0.cuda().requires_grad_()
    m, add = glue.mask_head(z, K, N, A, activation)
    assert m.shape == (K, B, N, E) and m.is_contiguous()
    close(f'{cfg} {activation} m', m, want_m.detach(), VALUE)
    if A:
        assert torch.equal(add.cpu().double(), want_a.detach())
        want_gz = torch.autograd.grad((want_m * gm.double()).sum() + (want_a * ga.double()).sum(), ref, retain_graph=True)[0]
        gz = torch.autograd.grad((m * gm.cuda()).sum() + (add * ga.cuda()).sum(), z, retain_graph=True)[0]
        close(f'{cfg} {activation} gz', gz, want_gz, GRAD)
        want_only = torch.autograd.grad((want_a * ga.double()).sum(), ref, retain_graph=True)[0]
        only = torch.autograd.grad((add * ga.cuda()).sum(), z, retain_graph=True)[0]       # the gradient of m is None
        close(f'{cfg} {activation} gz from additional alone', only, want_only, GRAD)
    else:
        assert add is None
    want_gz = torch.autograd.grad((want_m * gm.double()).sum(), ref)[0]
    gz = torch.autograd.grad((m * gm.cuda()).sum(), z)[0]                                   # g_additional is None
    close(f'{cfg} {activation} gz without g_additional', gz, want_gz, GRAD)
    if A:
        assert bool((gz[..., :A] == 0).all())


# ------------------------------------------------------------------------------------------------ centre and crop
def center_fp64(d, T):
    d = d[..., :T]
    return (d - d.mean(-1, keepdim=True)).transpose(0, 1)


@pytest.mark.parametrize('cfg', [(2, 3, 100, 100), (2, 3, 100, 92), (2, 3, 101, 90), (2, 3, 90, 100), (2, 2, 5, 1), (1, 1, 526340, 526340)],
                         ids=_id)
def test_center_against_fp64(cfg):
    from padertorch_amd.ops import tasnet as glue
    K, B, T_in, T = cfg
    gen = torch.Generator().manual_seed(154)
    d0 = torch.randn(K, B, T_in, generator=gen) + 0.3
    T_out = min(T, T_in)
    g = torch.randn(B, K, T_out, generator=gen)
    ref = d0.double().requires_grad_()
    want = center_fp64(ref, T)
    want_gd = torch.autograd.grad((want * g.double()).sum(), ref)[0]
    d = d0.cuda().requires_grad_()
    out = glue.center(d, T)
    assert out.shape == (B, K, T_out) and out.is_contiguous()
    gd = torch.autograd.grad((out * g.cuda()).sum(), d)[0]
    close(f'{cfg} centre out', out, want.detach(), VALUE)
    close(f'{cfg} centre gd', gd, want_gd, GRAD)
    assert bool((gd[..., T_out:] == 0).all())


# ------------------------------------------------------------------------------------------------ alignment and strides
SENTINEL, TAIL = 12345.0, 7


def unaligned(t):
    """A contiguous CUDA view of ``t``'s values one float into its storage (the vector kernels need 16 bytes), and the backing buffer."""
    n = t.numel()
    flat = torch.full((1 + n + TAIL,), SENTINEL, device='cuda')
    view = flat[1:1 + n].view(t.shape)
    view.copy_(t)
    assert view.is_contiguous() and view.data_ptr() % 16 == 4 and view.storage_offset() == 1
    return view, flat


def padding_untouched(name, flat):
    torch.cuda.synchronize()
    assert float(flat[0]) == SENTINEL and bool((flat[-TAIL:] == SENTINEL).all()), name


def _glue_call(op, x, extra, g):
    """(output(s), gradient of x) of one glue operator on the device tensor ``x``."""
    from padertorch_amd.ops import tasnet as glue
    x = x.requires_grad_()
    if op == 'entry_norm':
        outs = [glue.entry_norm(x, *extra)]
    elif op == 'prelu_rows':
        outs = [glue.prelu_rows(x, *extra)]
    elif op == 'mask_head':
        outs = list(glue.mask_head(x, *extra))
    else:
        outs = [glue.center(x, *extra)]
    gx = torch.autograd.grad(sum((o * w).sum() for o, w in zip(outs, g)), x)[0]
    return [o.detach() for o in outs], gx


def _glue_case(op, gen):
    if op == 'entry_norm':
        x = torch.randn(2, 128, 64, generator=gen)
        extra = (torch.rand(128, generator=gen).cuda() + 0.5, torch.rand(128, generator=gen).cuda() - 0.5, torch.tensor([64, 40]).cuda())
        g = [torch.randn(2, 64, 128, generator=gen).cuda()]
    elif op == 'prelu_rows':
        x, extra, g = dyadic(gen, (2, 70, 256), 1 / 8), (torch.tensor([0.25]).cuda(),), [torch.randn(2, 70, 256, generator=gen).cuda()]
    elif op == 'mask_head':
        x, extra = dyadic(gen, (2, 64, 4 + 2 * 64), 1 / 8), (2, 64, 4, 'sigmoid')
        g = [torch.randn(2, 2, 64, 64, generator=gen).cuda(), torch.randn(2, 4, 64, generator=gen).cuda()]
    else:
        x, extra, g = torch.randn(2, 3, 4096, generator=gen), (4000,), [torch.randn(3, 2, 4000, generator=gen).cuda()]
    return x, extra, g


@pytest.mark.parametrize('op', ['entry_norm', 'prelu_rows', 'mask_head', 'center'])
def test_unaligned_and_strided_inputs(op):
    """The input one float into its storage: the scalar kernels on that side, the same elementwise results bit for bit.  The gradient
    that comes in unaligned likewise.  A strided input is copied once and gives the same result."""
    gen = torch.Generator().manual_seed(155)
    x, extra, g = _glue_case(op, gen)
    outs0, gx0 = _glue_call(op, x.cuda(), extra, g)
    assert x.cuda().data_ptr() % 16 == 0
    view, flat = unaligned(x)
    outs, gx = _glue_call(op, view, extra, g)
    padding_untouched(op, flat)
    assert torch.equal(flat[1:1 + x.numel()].view(x.shape).cpu(), x)
    for a, b in zip(outs, outs0):
        assert torch.equal(a, b)
    assert torch.equal(gx, gx0)
    gview, gflat = unaligned(g[0])
    _, gx = _glue_call(op, x.cuda(), extra, [gview] + g[1:])
    padding_untouched(op + ' gradient', gflat)
    assert torch.equal(gx, gx0)
    wide = torch.zeros(x.shape[:-1] + (2 * x.shape[-1] + 1,), device='cuda')
    wide[..., 1::2] = x.cuda()
    strided = wide[..., 1::2]
    assert not strided.is_contiguous()
    outs, gx = _glue_call(op, strided.detach(), extra, g)
    for a, b in zip(outs, outs0):
        assert torch.equal(a, b)
    assert torch.equal(gx, gx0)
