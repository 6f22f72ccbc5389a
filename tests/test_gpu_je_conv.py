"""contrib/je's Conv1d, CNN1d and Pool1d on the GPU against the reference's fp64 run (tests/golden/g26_je_conv.npz) or the fp64 restatement
tests/je_conv_ref.py on the same inputs.

Gates (those of tests/test_gpu_je_rnn.py): values |diff| <= 1e-5 max|want|, gradients <= 2e-4 max|want|.  One exception: the gradient of
a convolution bias that a normalisation directly follows is zero in exact arithmetic; it is scaled by max|want| of the same convolution's
weight gradient (make_golden_je_conv.py).  The reference's own fp32 run stays within 0.056 of the gates on the fixture.  Every comparison
prints its ratio diff / (gate scale) (run with -s; profiles/je_conv_gates.txt is that output).  The full tensors are compared, the region
behind the lengths included.
"""
import copy
import importlib.util
import json
from pathlib import Path

import numpy as np
import pytest
import torch

import je_conv_ref as ref
from test_gpu_je_rnn import close, noncontiguous

pytestmark = pytest.mark.gpu

GOLDEN = Path(__file__).resolve().parent / 'golden'
VALUE, GRAD = 1e-5, 2e-4


@pytest.fixture(scope='module')
def g26():
    d = dict(np.load(GOLDEN / 'g26_je_conv.npz', allow_pickle=False))
    spec = importlib.util.spec_from_file_location('make_golden_je_conv', GOLDEN / 'make_golden_je_conv.py')
    d['maker'] = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(d['maker'])             # for the seeded inputs and the constructors (the reference is not imported)
    return d


def build(g, case):
    from padertorch_amd.contrib.je import modules as je
    cls, args, kwargs = g['maker'].CASES[case]
    net = getattr(je, cls)(*args, **kwargs)
    keys = json.loads(str(g[case + '_keys']))
    net.load_state_dict({k: torch.from_numpy(g[f'{case}_p_{k}']) for k in keys}, strict=True)
    return net.cuda()


def run(net, x, r, lengths):
    x = x.detach().requires_grad_()
    out = net(x, lengths)
    params = [p for p in net.parameters() if p.requires_grad]
    grads = torch.autograd.grad((out[0] * r).sum(), [x] + params)
    return out, [out[0].detach()] + list(grads)


def grad_scale(wants, name):
    """None (the gradient's own maximum) or, for a convolution bias whose fp64 gradient is zero against its weight's, that weight's."""
    want = wants[name]
    if name.endswith('conv.bias'):
        wscale = float(np.abs(wants[name[:-4] + 'weight']).max())
        if float(np.abs(want).max()) < 1e-9 * wscale:
            return wscale
    return None


# ---------------------------------------------------------------------------------------------------- the fixture through the modules
@pytest.mark.parametrize('case', ['c0', 'c1', 'c2', 'c3', 'c4', 'n0', 'n1', 'n2'])
def test_fixture_cases(g26, case):
    mk = g26['maker']
    net = build(g26, case)
    names = json.loads(str(g26[case + '_names']))
    assert names == [n for n, _ in net.named_parameters()]
    y_shape = g26[case + '_y64'].shape
    x0, r0 = mk.inputs(case, y_shape)
    x, r = torch.from_numpy(x0).cuda(), torch.from_numpy(r0).cuda()
    out, res = run(net, x, r, list(mk.LENGTHS))
    assert isinstance(out[1], np.ndarray) and out[1].dtype == np.int64 and np.array_equal(out[1], g26[case + '_len'])
    close(f'{case} y', res[0], g26[case + '_y64'], VALUE)
    close(f'{case} dx', res[1], g26[case + '_g64_x'], GRAD)
    wants = {n: g26[f'{case}_g64_{n}'] for n in names}
    for n, got in zip(names, res[2:]):
        close(f'{case} d {n}', got, wants[n], GRAD, grad_scale(wants, n))
    for form in (np.asarray(mk.LENGTHS), torch.tensor(mk.LENGTHS)):
        fresh = build(g26, case)
        for a, b in zip(res, run(fresh, noncontiguous(x0), r, form)[1]):
            assert torch.equal(a, b)
    with pytest.raises(NotImplementedError, match='GPU'):
        net(x, torch.tensor(mk.LENGTHS).cuda())
    if case == 'n0':
        # pool indices where the window's maximum is unique (judged on the restatement's fp64 windows)
        cpu = copy.deepcopy(build(g26, case)).cpu().double()
        _, _, indices = ref.cnn1d(cpu, torch.from_numpy(x0).double(), list(mk.LENGTHS))
        assert out[2][0] is None and out[2][2] is None and out[2][1].dtype == torch.int64
        assert np.array_equal(indices[1].numpy(), g26['n0_idx1'])
        assert torch.equal(out[2][1].cpu(), torch.from_numpy(g26['n0_idx1']))


def test_running_statistics_and_evaluation(g26):
    mk = g26['maker']
    net = build(g26, 'n0')
    x0, r0 = mk.inputs('n0', g26['n0_y64'].shape)
    x, r = torch.from_numpy(x0).cuda(), torch.from_numpy(r0).cuda()
    for _ in range(2):
        run(net, x, r, list(mk.LENGTHS))
    net.eval()
    out, res = run(net, x, r, list(mk.LENGTHS))
    close('n0 evaluation y', res[0], g26['n0e_y64'], VALUE)
    state = net.state_dict()
    for k in [k[len('n0e_b_'):] for k in g26 if k.startswith('n0e_b_')]:
        close('n0 buffer ' + k, state[k], g26['n0e_b_' + k], VALUE)
    # gradients in evaluation mode and with frozen statistics: against the restatement in the same state
    cpu = copy.deepcopy(net).cpu().double()
    xc = torch.from_numpy(x0).double().requires_grad_()
    yc = ref.cnn1d(cpu, xc, list(mk.LENGTHS))[0]
    want = torch.autograd.grad((yc * torch.from_numpy(r0).double()).sum(), [xc] + list(cpu.parameters()))
    names = [n for n, _ in net.named_parameters()]
    close('n0 evaluation dx', res[1], want[0], GRAD)
    for n, a, b in zip(names, res[2:], want[1:]):
        close('n0 evaluation d ' + n, a, b, GRAD)
    net.train()
    net.freeze(num_layers=2, freeze_norm_stats=True)
    before = {k: v.clone() for k, v in net.state_dict().items()}
    cpu = copy.deepcopy(net).cpu().double()
    out, res = run(net, x, r, list(mk.LENGTHS))
    yc = ref.cnn1d(cpu, xc, list(mk.LENGTHS))[0]
    close('n0 frozen y', res[0], yc.detach(), VALUE)
    want = torch.autograd.grad((yc * torch.from_numpy(r0).double()).sum(), [xc] + [p for p in cpu.parameters() if p.requires_grad])
    close('n0 frozen dx', res[1], want[0], GRAD)
    trainable = [n for n, p in net.named_parameters() if p.requires_grad]
    assert trainable and all(n.startswith(('convs.2', 'convs.3', 'residual_skip_convs')) for n in trainable), trainable
    wants = {n: w.numpy() for n, w in zip(trainable, want[1:])}
    for n, a in zip(trainable, res[2:]):
        close('n0 frozen d ' + n, a, wants[n], GRAD, grad_scale(wants, n))
    for k in before:
        if k.startswith(('convs.0.norm', 'convs.1.norm')):
            assert torch.equal(before[k], net.state_dict()[k]), k


@pytest.mark.parametrize('pad', ['both', 'front', 'end', None])
def test_fixture_pool(g26, pad):
    from padertorch_amd.contrib.je.modules import Pool1d
    mk = g26['maker']
    y64 = g26[f'q_{pad}_y64']
    x0, r0 = mk.pool_inputs(pad, y64.shape)
    for make in (lambda a: torch.from_numpy(a).cuda(), noncontiguous):
        x = make(x0).detach().requires_grad_()
        y, lens, idx = Pool1d('max', 3, 2, pad)(x, np.asarray(mk.POOL_LENGTHS))
        close(f'pool {pad} y', y, y64, VALUE)
        assert torch.equal(idx.cpu(), torch.from_numpy(g26[f'q_{pad}_idx'])) and np.array_equal(lens, g26[f'q_{pad}_len'])
        close(f'pool {pad} dx', torch.autograd.grad((y * torch.from_numpy(r0).cuda()).sum(), x)[0], g26[f'q_{pad}_g64_x'], GRAD)


# ---------------------------------------------------------------------------------------------------- against the restatement
def against_restatement(name, net, x0, lengths, seed=0, is_cnn=False, x=None):
    """``net`` (on the GPU) on ``x0`` against the restatement of its CPU fp64 copy: values and every gradient."""
    fn = ref.cnn1d if is_cnn else ref.conv1d
    cpu = copy.deepcopy(net).cpu().double()
    xc = torch.from_numpy(x0).double().requires_grad_()
    yc = fn(cpu, xc, lengths)[0]
    r0 = np.random.RandomState(seed).randn(*yc.shape).astype(np.float32)
    want = torch.autograd.grad((yc * torch.from_numpy(r0).double()).sum(), [xc] + list(cpu.parameters()))
    x = torch.from_numpy(x0).cuda() if x is None else x
    out, res = run(net, x, torch.from_numpy(r0).cuda(), lengths)
    close(name + ' y', res[0], yc.detach(), VALUE)
    close(name + ' dx', res[1], want[0], GRAD)
    wants = {n: w.numpy() for (n, _), w in zip(net.named_parameters(), want[1:])}
    for (n, _), got in zip(net.named_parameters(), res[2:]):
        close(f'{name} d {n}', got, wants[n], GRAD, grad_scale(wants, n))
    return res


def perturbed(net, seed=1):
    rng = np.random.RandomState(seed)
    with torch.no_grad():
        for n, p in net.named_parameters():
            if n.endswith(('bias', 'gamma', 'beta', 'activation_fn.weight')):
                p.add_(torch.from_numpy(0.3 * rng.randn(*p.shape)).float())
    return net.cuda()


#: name -> (C_in, C_out, K, keyword arguments, (B, T), lengths)
SHAPES = {
    'scalar path 7 -> 10': (7, 10, 3, dict(norm='batch', gated=True, activation_fn='elu'), (2, 19), [19, 11]),
    'scalar path 10 -> 7, pre': (10, 7, 3, dict(norm='sequence', pre_activation=True, activation_fn='sigmoid', dilation=2), (2, 19), [13, 19]),
    'tiles 130 -> 70': (130, 70, 3, dict(norm='batch', activation_fn='prelu', stride=2), (2, 37), [37, 20]),
    'row tile T = 1030': (4, 4, 3, dict(norm='batch', gated=True), (2, 1030), [1030, 517]),
    'T_out = 1': (4, 8, 5, dict(pad_type=None, norm='sequence', activation_fn='tanh'), (3, 5), [5, 5, 5]),
    'a sequence of length 1': (4, 8, 3, dict(norm='batch', activation_fn='leaky_relu'), (3, 9), [9, 1, 4]),
    'stride above the kernel': (8, 8, 2, dict(stride=3, norm='batch'), (2, 17), [17, 8]),
    'stride above the kernel, front': (8, 8, 2, dict(stride=3, pad_type='front', gated=True), (2, 17), None),
    'K = 1': (8, 12, 1, dict(norm='sequence', gated=True), (2, 9), [9, 3]),
    'front pad above T_in': (4, 4, 4, dict(dilation=3, pad_type='front', norm='batch'), (2, 5), [5, 2]),
    'end pad, no norm, no bias': (6, 5, 4, dict(dilation=2, pad_type='end', bias=False, activation_fn='identity'), (2, 9), None),
}


@pytest.mark.parametrize('name', sorted(SHAPES))
def test_conv1d_against_restatement(name):
    from padertorch_amd.contrib.je.modules import Conv1d
    C_in, C_out, K, kwargs, (B, T), lengths = SHAPES[name]
    torch.manual_seed(3)
    net = perturbed(Conv1d(C_in, C_out, K, **kwargs))
    x0 = np.random.RandomState(5).randn(B, C_in, T).astype(np.float32)
    res = against_restatement(name, net, x0, lengths)
    for a, b in zip(res, against_restatement(name + ', non-contiguous input', net, x0, lengths, x=noncontiguous(x0))):
        assert torch.equal(a, b)


def test_a_channel_slice_of_wider_rows_is_read_in_place():
    """``x = unrows(wide rows)[:, :C]``: rows with a leading dimension above their width, read without a copy by the statistics, apply,
    taps (residual) and pool kernels, the pack pass and the scale word; the same bits as the contiguous run, gradients included."""
    from padertorch_amd.contrib.je.modules import Conv1d, Pool1d
    from padertorch_amd.ops import je_conv
    B, T, C, W = 2, 21, 8, 12
    rng = np.random.RandomState(13)
    wide = torch.from_numpy(rng.randn(B * T, W).astype(np.float32)).cuda()
    res_wide = torch.from_numpy(rng.randn(B * T, W).astype(np.float32)).cuda()
    view, res_view = (je_conv.unrows(w, B, T)[:, 2:2 + C] for w in (wide, res_wide))          # (offset 2: not 16-byte aligned)
    aligned = je_conv.unrows(wide, B, T)[:, 4:4 + C]
    for v in (view, aligned):
        r, _, _ = je_conv.rows(v)
        assert r.stride() == (W, 1) and r.data_ptr() == v.data_ptr()                           # in place, no gather
    torch.manual_seed(8)
    net = perturbed(Conv1d(C, C, 3, norm='batch', pre_activation=True, gated=True, activation_fn='elu'))
    post = perturbed(Conv1d(C, C, 3, norm='sequence'), seed=2)
    pool = Pool1d('max', 3, 2, 'both')
    r = torch.from_numpy(rng.randn(B, C, T).astype(np.float32)).cuda()

    def go(x, res):
        x = x.detach().requires_grad_()
        y = net(x, [21, 12], _residual=res)[0]
        y2 = post(x, [21, 12])[0]
        y3, _, idx = pool(x)
        grads = torch.autograd.grad((y * r).sum() + (y2 * r).sum() + y3.sum(), [x] + list(net.parameters()) + list(post.parameters()))
        return [y.detach(), y2.detach(), y3.detach(), idx] + list(grads)
    for v in (view, aligned):
        for a, b in zip(go(v, res_view), go(v.contiguous(), res_view.contiguous())):
            assert a.shape == b.shape and torch.equal(a, b)


def test_cnn1d_against_restatement_with_several_residuals():
    from padertorch_amd.contrib.je.modules import CNN1d
    torch.manual_seed(4)
    net = perturbed(CNN1d(5, [8, 8, 8, 6], [3, 2, 3, 1], residual_connections=[None, [2, 3], 3, None], dense_connections=[1, None, None, None],
                          norm='batch', activation_fn=['identity', 'relu', 'prelu', 'tanh', 'identity'], stride=[1, 2, 1, 1],
                          pool_type=['max', None, 'avg', None], pool_size=[2, 1, 3, 1], pool_stride=[2, 1, 2, 1], pre_activation=True,
                          input_layer=True, output_layer=False))
    x0 = np.random.RandomState(6).randn(3, 5, 41).astype(np.float32)
    against_restatement('cnn1d', net, x0, [41, 30, 24], is_cnn=True)


def test_nan_behind_a_length_does_not_reach_the_statistics():
    from padertorch_amd.contrib.je.modules import Conv1d
    torch.manual_seed(5)
    net = perturbed(Conv1d(4, 6, 1, norm='batch', pad_type=None))
    x0 = np.random.RandomState(7).randn(2, 4, 9).astype(np.float32)
    clean = net(torch.from_numpy(x0).cuda(), [9, 5])[0]
    x0[1, :, 6] = np.nan
    y = net(torch.from_numpy(x0).cuda(), [9, 5])[0]
    assert torch.equal(y[1, :, 5:], torch.zeros_like(y[1, :, 5:])) and torch.isfinite(y).all()
    # A departure from the reference, NOT asserted (conv.py's docstring): the NaN enters the operand scale of the planes
    # GEMM (ops.gemm takes a non-finite maximum as the largest finite float), which spoils the whole call's output in front of the
    # lengths: measured on an MI355X at 9.9e4 of the value gate against the clean call, that is about max|y| itself.
    print('NaN behind a length, the rest of the output against the clean call: max |diff| %.3e' % float((y - clean).detach().abs().max()))


# ---------------------------------------------------------------------------------------------------- determinism and capture
def test_backward_twice_gives_equal_bits(g26):
    mk = g26['maker']
    net = build(g26, 'n0')
    x0, r0 = mk.inputs('n0', g26['n0_y64'].shape)
    x, r = torch.from_numpy(x0).cuda(), torch.from_numpy(r0).cuda()
    state = copy.deepcopy(net.state_dict())
    first = run(net, x, r, list(mk.LENGTHS))[1]
    net.load_state_dict(state)
    for a, b in zip(first, run(net, x, r, list(mk.LENGTHS))[1]):
        assert torch.equal(a, b)


def test_capture_replays_equal_eager_bit_for_bit(g26):
    mk = g26['maker']
    net = build(g26, 'n2')
    x0, r0 = mk.inputs('n2', g26['n2_y64'].shape)
    x, r = torch.from_numpy(x0).cuda(), torch.from_numpy(r0).cuda()
    state = copy.deepcopy(net.state_dict())
    run(net, x, r, None)                                                  # warm-up: every cache is filled
    sx, sr = x.clone(), r.clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run(net, sx, sr, None)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        captured = run(net, sx, sr, None)[1]
    for seed in (11, 12):
        rng = np.random.RandomState(seed)
        nx, nr = (torch.from_numpy((3 * rng.randn(*t.shape)).astype(np.float32)).cuda() for t in (x, r))
        sx.copy_(nx)
        sr.copy_(nr)
        graph.replay()
        torch.cuda.synchronize()
        net.load_state_dict(state)                                       # (the running statistics do not enter a training pass)
        for k, (a, b) in enumerate(zip(captured, run(net, nx, nr, None)[1])):
            assert torch.equal(a, b), ('replay', seed, k)


# ---------------------------------------------------------------------------------------------------- with the recurrent wrappers
def test_gru_with_a_cnn1d_output_net():
    import je_rnn_ref
    from padertorch_amd.contrib.je import modules as je
    torch.manual_seed(6)
    gru = torch.nn.GRU(5, 6, 1, batch_first=True, bidirectional=True)
    cnn = perturbed(je.CNN1d(12, [8, 4], 3, norm='batch', gated=True))
    net = je.GRU(gru, output_net=cnn).cuda()
    lengths = [13, 9, 4]
    x0 = np.random.RandomState(8).randn(3, 5, 13).astype(np.float32)
    cpu = copy.deepcopy(net).cpu().double()
    xc = torch.from_numpy(x0).double().requires_grad_()
    dirs = [tuple(getattr(cpu.rnn, f'{n}_l0{s}') for n in ('weight_ih', 'weight_hh', 'bias_ih', 'bias_hh')) for s in ('', '_reverse')]
    h = je_rnn_ref.gru_stack(xc, lengths, [dirs])
    yc = ref.cnn1d(cpu.output_net, h, lengths)[0]
    r0 = np.random.RandomState(9).randn(*yc.shape).astype(np.float32)
    want = torch.autograd.grad((yc * torch.from_numpy(r0).double()).sum(), [xc] + list(cpu.parameters()))
    (y, lens), res = run(net, torch.from_numpy(x0).cuda(), torch.from_numpy(r0).cuda(), lengths)
    assert np.array_equal(lens, lengths)
    close('gru + cnn1d y', res[0], yc.detach(), VALUE)
    close('gru + cnn1d dx', res[1], want[0], GRAD)
    wants = {n: w.numpy() for (n, _), w in zip(net.named_parameters(), want[1:])}
    for (n, _), got in zip(net.named_parameters(), res[2:]):
        close('gru + cnn1d d ' + n, got, wants[n], GRAD, grad_scale(wants, n))
