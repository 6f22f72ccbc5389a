"""``Conv2d``, ``CNN2d``, ``Pool2d`` and the hybrids (``csrc/je_conv2d.hip``) against the reference's own modules in fp64 (``golden/g27``)
and, for configurations outside the fixture, against torch's own ``F.conv2d`` / ``F.max_pool2d`` / ``F.avg_pool2d`` in fp64
on the CPU.  Gates as in ``test_gpu_je_conv.py``: values ``1e-5 max|want|``, gradients ``2e-4 max|want|``; a convolution bias directly in
front of a normalisation is scaled by its weight's gradient.  Full tensors are compared, the region behind the lengths included, and
every comparison prints its ratio (``profiles/je_conv2d_gates.txt``)."""
import copy
import importlib.util
import json
from pathlib import Path

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from test_gpu_je_conv import GRAD, VALUE, grad_scale
from test_gpu_je_rnn import close, noncontiguous

pytestmark = pytest.mark.gpu
GOLDEN = Path(__file__).resolve().parent / 'golden'

B, F_IN, T_IN, LENGTHS = 3, 12, 21, [21, 17, 9]


def pads(net):
    from padertorch_amd.contrib.je.modules import compute_pad_size
    (ff, fe), (tf, te) = (compute_pad_size(k, d, s, p) for k, d, s, p in zip(net.kernel_size, net.dilation, net.stride, net.pad_type))
    return tf, te, ff, fe


def norm_act64(net, v, lengths):
    """``activation_fn(norm(v))`` of a block in plain torch: masked statistics over ``t < len_b`` ('batch': over b, f, t; 'sequence': over t)."""
    if net.norm is not None:
        mask = (torch.arange(v.shape[3])[None] < torch.as_tensor(lengths)[:, None]).double()[:, None, None, :]
        axes = (0, 2, 3) if net.norm.track_running_stats else (3,)
        count = (mask.expand(-1, 1, v.shape[2], -1)).sum(axes, keepdim=True).clamp(min=1)
        mean = (v * mask).sum(axes, keepdim=True) / count
        var = ((v * mask) ** 2).sum(axes, keepdim=True) / count - mean ** 2
        v = (net.norm.gamma * (v - mean) / torch.sqrt(var.clamp(min=0) + net.norm.eps) + net.norm.beta) * mask
    return net.activation_fn(v)


def block64(net, x, lengths, residual=None):
    """One ``Conv2d`` block (a CPU fp64 copy of the module holds the parameters) as ``F.pad`` + ``F.conv2d`` + the lines above."""
    a = norm_act64(net, x, lengths) if net.pre_activation else x
    a = F.pad(a, pads(net))
    z = F.conv2d(a, net.conv.weight, net.conv.bias, net.stride, 0, net.dilation)
    if not net.pre_activation:
        z = norm_act64(net, z, lengths if lengths is None else net.get_output_sequence_lengths(lengths))
    if net.gated:
        z = z * torch.sigmoid(F.conv2d(a, net.gate_conv.weight, net.gate_conv.bias, net.stride, 0, net.dilation))
    return z if residual is None else z + residual


def check(name, net, want_fn, run_fn, x0, extra=()):
    """Values and every gradient of ``run_fn(net on the GPU, x, *extra)`` against ``want_fn(its fp64 copy, x, *extra)``; returns the GPU's
    ``(y, [dx, every parameter gradient])``."""
    cpu = copy.deepcopy(net).cpu().double()
    xc = torch.from_numpy(x0).double().requires_grad_()
    ec = [torch.from_numpy(e).double() for e in extra]
    yc = want_fn(cpu, xc, *ec)
    r0 = np.random.RandomState(5).randn(*yc.shape).astype(np.float32)
    want = torch.autograd.grad((yc * torch.from_numpy(r0).double()).sum(), [xc] + list(cpu.parameters()))
    x = torch.from_numpy(x0).cuda().requires_grad_()
    y = run_fn(net, x, *[torch.from_numpy(e).cuda() for e in extra])
    got = torch.autograd.grad((y * torch.from_numpy(r0).cuda()).sum(), [x] + list(net.parameters()))
    close(name + ' y', y, yc.detach(), VALUE)
    close(name + ' dx', got[0], want[0], GRAD)
    wants = {n: w.numpy() for (n, _), w in zip(net.named_parameters(), want[1:])}
    for (n, _), g in zip(net.named_parameters(), got[1:]):
        close(f'{name} d {n}', g, wants[n], GRAD, grad_scale(wants, n))
    return y, list(got)


def perturbed(net, seed=1):
    rng = np.random.RandomState(seed)
    with torch.no_grad():
        for n, p in net.named_parameters():
            if n.endswith(('bias', 'gamma', 'beta')):
                p.add_(torch.from_numpy(0.3 * rng.randn(*p.shape)).float())
    return net.cuda()


NORMS = {f'{norm}{", pre" if pre else ""}': dict(norm=norm, activation_fn='relu', pre_activation=pre)
         for norm in ('batch', 'sequence') for pre in (False, True)}
#: one thing at a time away from 8 -> 16, 3 x 3, stride 1, pad 'both', no norm, identity: (C_in, C_out, kernel, keyword arguments)
BLOCKS = {
    **{f'C_in {c}': (c, 16, 3, {}) for c in (8, 1, 3, 11, 40)},
    **{f'C_out {c}': (8, c, 3, {}) for c in (5, 10, 144)},
    'kernel (2, 2), no pad': (8, 16, (2, 2), dict(pad_type=None)),
    **{f'kernel {k}': (8, 16, k, {}) for k in ((1, 1), (3, 1), (1, 5))},
    **{f'stride {s}': (8, 16, 3, dict(stride=s)) for s in ((2, 1), (2, 2))},
    **{f'dilation {d}': (8, 16, 3, dict(dilation=d)) for d in ((2, 1), (1, 3))},
    **{f'pad {p}': (8, 16, 3, dict(pad_type=p)) for p in (('front', 'end'), (None, 'both'))},
    'kernel (1, 1), C_in 72': (72, 16, (1, 1), {}),          # the weight gradient's LDS beyond 64 KB
    'gated': (8, 16, 3, dict(gated=True)),
    **{k: (8, 16, 3, v) for k, v in NORMS.items()},
    'residual': (8, 16, 3, dict(residual=True)),
    'gated, batch norm, stride 2, residual': (11, 10, 3, dict(gated=True, norm='batch', activation_fn='elu', stride=2, residual=True)),
}


@pytest.mark.parametrize('name', list(BLOCKS))
def test_block_against_conv2d_fp64(name):
    from padertorch_amd.contrib.je.modules import Conv2d
    c_in, c_out, kernel, kwargs = BLOCKS[name]
    kwargs = dict({'activation_fn': 'identity'}, **kwargs)
    has_residual = kwargs.pop('residual', False)
    torch.manual_seed(3)
    net = perturbed(Conv2d(c_in, c_out, kernel, **kwargs))
    rng = np.random.RandomState(2)
    x0 = rng.randn(B, c_in, F_IN, T_IN).astype(np.float32)
    shape = tuple(int(n) for n in net.get_output_shape(x0.shape))
    extra = [rng.randn(*shape).astype(np.float32)] if has_residual else []
    check(name, net, lambda m, x, *r: block64(m, x, LENGTHS, *r),
          lambda m, x, *r: m(x, LENGTHS, _residual=r[0] if r else None)[0], x0, extra)


def test_weight_gradient_slabs():
    """A plane large enough for several slabs: the planner says so, and ``dW`` is the fp64 one."""
    from padertorch_amd.contrib.je.modules import Conv2d
    from padertorch_amd.ops.je_conv2d import wgrad_slabs
    assert wgrad_slabs(2, 40, 150, 1, 16, 8, 9) >= 2
    torch.manual_seed(4)
    net = Conv2d(8, 16, 3, activation_fn='identity').cuda()
    x0 = np.random.RandomState(6).randn(2, 8, 40, 150).astype(np.float32)
    check('slabs', net, lambda m, x: block64(m, x, None), lambda m, x: m(x)[0], x0)


POOLS = [(size, stride, pad, C) for size, stride in (((2, 2), None), ((1, 3), None), ((3, 2), None), ((2, 2), (1, 2)))
         for pad in (None, 'both', ('front', None)) for C in (5, 8)]


@pytest.mark.parametrize('pool_type', ['max', 'avg'])
@pytest.mark.parametrize('size,stride,pad,C', POOLS)
def test_pool2d(pool_type, size, stride, pad, C):
    """Standard-normal input has no ties: every window, the int64 indices, the output lengths and ``dx``."""
    from padertorch_amd.contrib.je.modules import Pool2d, compute_pad_size, to_pair
    x0 = np.random.RandomState(8).randn(B, C, F_IN, T_IN).astype(np.float32)
    front, end = zip(*[compute_pad_size(k, 1, k, p) for k, p in zip(size, to_pair(pad))])
    xc = torch.from_numpy(x0).double().requires_grad_()
    xp = F.pad(xc, (front[1], end[1], front[0], end[0]))
    eff = to_pair(size if stride is None else stride)
    trim = [max(n - k, 0) % s for n, k, s in zip(xp.shape[2:], size, eff)]
    xp = xp[:, :, :xp.shape[2] - trim[0], :xp.shape[3] - trim[1]]
    yc, ic = F.max_pool2d(xp, size, eff, return_indices=True) if pool_type == 'max' else (F.avg_pool2d(xp, size, eff), None)
    x = torch.from_numpy(x0).cuda().requires_grad_()
    y, lengths, index = Pool2d(pool_type, size, stride, pad)(x, LENGTHS)
    name = f'{pool_type} pool {size} / {stride}, pad {pad}, C {C}'
    close(name + ' y', y, yc.detach(), VALUE)
    tf, te = compute_pad_size(size[1], 1, eff[1], to_pair(pad)[1])
    assert np.array_equal(lengths, 1 + (np.array(LENGTHS) + tf + te - size[1]) // eff[1])
    assert (index is None) == (ic is None) and (ic is None or (index.dtype == torch.int64 and torch.equal(index.cpu(), ic)))
    r = torch.from_numpy(np.random.RandomState(9).randn(*yc.shape).astype(np.float32))
    close(name + ' dx', torch.autograd.grad((y * r.cuda()).sum(), x)[0], torch.autograd.grad((yc * r.double()).sum(), xc)[0], GRAD)


@pytest.fixture(scope='module')
def g27():
    d = dict(np.load(GOLDEN / 'g27_je_conv2d.npz', allow_pickle=False))
    spec = importlib.util.spec_from_file_location('make_golden_je_conv2d', GOLDEN / 'make_golden_je_conv2d.py')
    d['maker'] = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(d['maker'])             # for the seeded inputs and the constructors (the reference is not imported)
    return d


def build(g, case):
    from padertorch_amd.contrib.je import modules as je
    from padertorch_amd.modules.fully_connected import fully_connected_stack
    mods = {'CNN2d': je.CNN2d, 'CNN1d': je.CNN1d, 'CNN': je.hybrid.CNN, 'CRNN': je.hybrid.CRNN, 'GRU': torch.nn.GRU,
            'fully_connected_stack': fully_connected_stack}
    cls, *spec = g['maker'].CASES[case]
    net = mods[cls](*spec[0], **spec[1]) if len(spec) == 2 else g['maker'].assemble(cls, spec[0], mods)
    keys = json.loads(str(g[case + '_keys']))
    net.load_state_dict({k: torch.from_numpy(g[f'{case}_p_{k}']) for k in keys}, strict=True)
    return net.cuda()


def run(g, case, net, x, lengths):
    """``[y, dx, every parameter gradient]`` and the whole output tuple."""
    mk = g['maker']
    cond = mk.inputs(case)[1]
    x = x.detach().requires_grad_()
    out = net(x, lengths, torch.from_numpy(cond).cuda()) if cond is not None else net(x, lengths)
    r = torch.from_numpy(mk.inputs(case, tuple(out[0].shape))[2]).cuda()
    return out, [out[0].detach()] + list(torch.autograd.grad((out[0] * r).sum(), [x] + list(net.parameters())))


@pytest.mark.parametrize('case', ['w0', 'w1', 'w2', 'h0', 'h1'])
def test_fixture_cases(g27, case):
    """The reference's own modules in fp64 (g27): strict load, parameter order, ``y``, lengths, ``dx``, every parameter gradient, pool
    indices; then a non-contiguous input and the other forms of lengths give the same bits."""
    mk = g27['maker']
    net = build(g27, case)
    names = json.loads(str(g27[case + '_names']))
    assert names == [n for n, _ in net.named_parameters()]
    x0 = mk.inputs(case)[0]
    out, res = run(g27, case, net, torch.from_numpy(x0).cuda(), list(mk.LENGTHS))
    assert isinstance(out[1], np.ndarray) and out[1].dtype == np.int64 and np.array_equal(out[1], g27[case + '_len'])
    close(f'{case} y', res[0], g27[case + '_y64'], VALUE)
    close(f'{case} dx', res[1], g27[case + '_g64_x'], GRAD)
    wants = {n: g27[f'{case}_g64_{n}'] for n in names}
    for n, got in zip(names, res[2:]):
        close(f'{case} d {n}', got, wants[n], GRAD, grad_scale(wants, n))
    if case == 'w2':
        assert out[2][1] is None and out[2][0].dtype == torch.int64 and np.array_equal(out[2][0].cpu().numpy(), g27['w2_idx0'])
    for form in (np.asarray(mk.LENGTHS), torch.tensor(mk.LENGTHS)):
        for a, b in zip(res, run(g27, case, build(g27, case), noncontiguous(x0), form)[1]):
            assert torch.equal(a, b)


def test_evaluation_after_two_training_steps(g27):
    mk = g27['maker']
    net = build(g27, 'w0')
    x = torch.from_numpy(mk.inputs('w0')[0]).cuda()
    for _ in range(2):
        run(g27, 'w0', net, x, list(mk.LENGTHS))
    net.eval()
    with torch.no_grad():
        close('w0 evaluation y', net(x, list(mk.LENGTHS))[0], g27['w0e_y64'], VALUE)
    state = net.state_dict()
    for k in state:
        if 'running' in k or 'num_tracked' in k:
            close('w0 buffer ' + k, state[k], g27['w0e_b_' + k], VALUE)


def capture(g27):
    """Forward + backward of the first fixture case without lengths captured in a plain ``torch.cuda.graph``: ``(net, graph, its static
    x and r, its outputs, the eager step)``."""
    net = build(g27, 'w0')
    params = list(net.parameters())
    sx = torch.zeros(B, 1, F_IN, T_IN).cuda().requires_grad_()
    sr = torch.zeros(*g27['w0_y64'].shape).cuda()

    def step(x, r):
        y = net(x)[0]
        return [y] + list(torch.autograd.grad((y * r).sum(), [x] + params))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step(sx, sr)                                                    # warm-up: every cache is filled
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        captured = step(sx, sr)
    return net, graph, sx, sr, captured, step


def test_graph_replays_bit_identically(g27):
    """Replays on new inputs against the eager call (the operand scale words start from zero in every replay)."""
    _, graph, sx, sr, captured, step = capture(g27)
    for seed, scale in ((11, 3.), (12, .01), (13, 1.)):
        rng = np.random.RandomState(seed)
        nx, nr = (torch.from_numpy((scale * rng.randn(*t.shape)).astype(np.float32)).cuda() for t in (sx, sr))
        with torch.no_grad():
            sx.copy_(nx)
            sr.copy_(nr)
        graph.replay()
        torch.cuda.synchronize()
        for k, (a, b) in enumerate(zip(captured, step(nx.requires_grad_(), nr))):
            assert torch.equal(a, b), ('replay', seed, k)


def test_graph_replay_follows_a_weight_update(g27):
    """The weight planes are packed inside the graph: after an in-place update of every parameter the replay gives the bits of the eager
    call with the updated weights (several replays), not those of the weights it was captured with."""
    net, graph, sx, sr, captured, step = capture(g27)
    rng = np.random.RandomState(14)
    nx, nr = (torch.from_numpy(rng.randn(*t.shape).astype(np.float32)).cuda() for t in (sx, sr))
    with torch.no_grad():
        sx.copy_(nx)
        sr.copy_(nr)
    graph.replay()
    torch.cuda.synchronize()
    before = [t.clone() for t in captured]
    gen = torch.Generator().manual_seed(15)
    for _ in range(2):
        with torch.no_grad():
            for p in net.parameters():
                p.add_((0.1 * torch.randn(p.shape, generator=gen)).cuda())
        graph.replay()
        torch.cuda.synchronize()
        for k, (a, b) in enumerate(zip(captured, step(nx.requires_grad_(), nr))):
            assert torch.equal(a, b), ('replay after a weight update', k)
        assert not torch.equal(captured[0], before[0]) and not torch.equal(captured[1], before[1])
