"""``ConvTranspose1d`` / ``ConvTranspose2d``, ``Unpool1d`` / ``Unpool2d`` and the ``CNNTranspose*`` stacks (``csrc/je_conv_transpose.hip``)
against plain torch in fp64 on the CPU: ``F.conv_transpose*``, the slice ``compute_pad_size`` gives, then the norm / activation / gate
lines with the reference's quirk (the UNTRIMMED output is normalised with the TRIMMED lengths); ``F.max_unpool*`` / ``F.interpolate``.
The project's standing gates: values ``1e-5 max|want|``, gradients ``2e-4 max|want|``."""
from pathlib import Path

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from test_gpu_je_conv import GRAD, VALUE
from test_gpu_je_conv2d import check, close, perturbed

pytestmark = pytest.mark.gpu


def mods():
    from padertorch_amd.contrib.je.modules import conv_transpose
    return conv_transpose


def norm_act64(net, v, lengths):
    """``activation_fn(norm(v))`` on ``v [B, C, F, T]`` in plain torch: masked statistics over ``t < len_b`` ('batch': over b, f, t;
    'sequence': over t), or in evaluation mode the running statistics; zeros behind the lengths."""
    n = net.norm
    if n is not None:
        mask = (torch.arange(v.shape[3])[None] < torch.as_tensor(lengths)[:, None]).double()[:, None, None, :]
        if n.track_running_stats and not net.training:
            mean, var = n.running_mean.view(1, -1, 1, 1), n.running_var.view(1, -1, 1, 1)
        else:
            axes = (0, 2, 3) if n.track_running_stats else (3,)
            count = (mask.expand(-1, 1, v.shape[2], -1)).sum(axes, keepdim=True).clamp(min=1)
            mean = (v * mask).sum(axes, keepdim=True) / count
            var = (((v * mask) ** 2).sum(axes, keepdim=True) / count - mean ** 2).clamp(min=0)
        v = (n.gamma.view(1, -1, 1, 1) * (v - mean) / torch.sqrt(var + n.eps) + n.beta.view(1, -1, 1, 1)) * mask
    return net.activation_fn(v)


def block64(net, x, lengths, residual=None):
    """One transposed block (a CPU fp64 copy holds the parameters) on ``x [B, C, F, T]``; a 1-D block's weights get a unit ``f`` axis."""
    from padertorch_amd.contrib.je.modules import compute_pad_size
    kernel, stride, dilation, pad = net._axes()
    w4 = (lambda w: w) if net.is_2d() else (lambda w: w.unsqueeze(2))
    na = norm_act64
    a = na(net, x, lengths) if net.pre_activation else x
    z = F.conv_transpose2d(a, w4(net.conv.weight), net.conv.bias, stride, 0, 0, 1, dilation)
    if not net.pre_activation:
        z = na(net, z, net.get_output_sequence_lengths(lengths))          # untrimmed plane, trimmed lengths
    if net.gated:
        z = z * torch.sigmoid(F.conv_transpose2d(a, w4(net.gate_conv.weight), net.gate_conv.bias, stride, 0, 0, 1, dilation))
    (ff, fe), (tf, te) = (compute_pad_size(k, d, s, p) for k, d, s, p in zip(kernel, dilation, stride, pad))
    z = z[:, :, ff:z.shape[2] - max(fe - stride[0] + 1, 0), tf:z.shape[3] - max(te - stride[1] + 1, 0)]
    return z if residual is None else z + residual


S22 = dict(stride=(2, 2))
#: name -> (C_in, C_out, kernel, keyword arguments, input plane); a plane of one number: the 1-D class
CASES = {
    **{f'phases {s}/{k}/{d}': (8, 16, k, dict(stride=s, dilation=d), (5, 9)) for s, k, d in (
        ((1, 1), 3, 1), ((2, 2), 3, 1), ((2, 3), 3, 1), ((2, 2), 4, 1), ((3, 3), 2, 1), ((2, 2), 3, 2), ((2, 2), 3, 3), ((1, 2), (1, 5), 1))},
    **{f'trim {p}/{k}': (8, 16, k, dict(S22, pad_type=p), (5, 9)) for p in (None, 'both', 'front', ('front', 'end')) for k in (3, 4)},
    **{f'plane {p}': (8, 16, 3, S22, p) for p in ((8, 16), (7, 15), (9, 17), (1, 1))},
    **{f'T_in {t}': (8, 16, 4, dict(stride=2), (t,)) for t in (1, 127, 128, 129)},
    **{f'C_in {c}': (c, 16, 3, S22, (5, 9)) for c in (1, 33)},
    **{f'C_out {c}': (8, c, 3, S22, (5, 9)) for c in (1, 65)},
    'gated': (8, 16, 3, dict(S22, gated=True), (9, 17)),
    'residual': (8, 16, 3, dict(S22, residual=True), (9, 17)),
    'batch norm': (8, 16, 4, dict(S22, norm='batch', activation_fn='relu'), (9, 17)),
    'batch norm, fixed': (8, 16, 4, dict(S22, norm='batch', activation_fn='relu', fixed=True), (9, 17)),
    'sequence norm': (8, 16, 4, dict(S22, norm='sequence', activation_fn='relu'), (9, 17)),
    'batch norm, pre': (8, 16, 4, dict(S22, norm='batch', activation_fn='relu', pre_activation=True), (9, 17)),
    # (kernel 4 at stride 2 with 'both': front = 1, so the untrimmed plane's statistics and the early zeros are exercised)
    'prelu': (8, 16, 3, dict(S22, activation_fn='prelu'), (9, 17)),
    'gated, sequence norm, 1-D, residual': (8, 16, 3, dict(stride=2, gated=True, norm='sequence', activation_fn='elu', residual=True), (17,)),
}


@pytest.mark.parametrize('name', list(CASES))
def test_block_against_conv_transpose_fp64(name):
    """Values, ``dx`` and every parameter gradient of one block, ``B = 2``, lengths ``[T, T // 2]``."""
    c_in, c_out, kernel, kwargs, plane = CASES[name]
    kwargs = dict({'activation_fn': 'identity'}, **kwargs)
    has_residual, fixed = kwargs.pop('residual', False), kwargs.pop('fixed', False)
    torch.manual_seed(3)
    net = perturbed((mods().ConvTranspose2d if len(plane) == 2 else mods().ConvTranspose1d)(c_in, c_out, kernel, **kwargs))
    rng = np.random.RandomState(2)
    if fixed:
        with torch.no_grad():
            net.norm.running_mean.add_(torch.from_numpy(0.3 * rng.randn(*net.norm.running_mean.shape)).float().cuda())
            net.norm.running_var.mul_(1.7)
        net.eval()
    x0 = rng.randn(2, c_in, *plane).astype(np.float32)
    lengths = [plane[-1], max(plane[-1] // 2, 1)]
    extra = [rng.randn(*net.get_output_shape(x0.shape)).astype(np.float32)] if has_residual else []
    up = (lambda t: t) if len(plane) == 2 else (lambda t: t.unsqueeze(2))
    y, _ = check(name, net, lambda m, x, *r: block64(m, up(x), lengths, *[up(e) for e in r]).reshape(net.get_output_shape(x0.shape).tolist()),
                 lambda m, x, *r: m(x, lengths, _residual=r[0] if r else None)[0], x0, extra)
    assert np.array_equal(net(torch.from_numpy(x0).cuda(), lengths)[1], net.get_output_sequence_lengths(lengths))


UNPOOLS = [(size, stride, pad, plane) for size, stride in ((2, None), (2, 3), ((2, 2), None), ((3, 2), None), ((2, 2), (2, 3)))
           for pad in (None, 'both') for plane in ((21,) if np.isscalar(size) else (12, 21),)]


@pytest.mark.parametrize('with_indices', [True, False])
@pytest.mark.parametrize('size,stride,pad,plane', UNPOOLS)
def test_unpool_round_trip(size, stride, pad, plane, with_indices):
    """Through this package's max pool and back: values, ``dx`` and the output lengths against ``F.max_unpool*`` + the reference's trim, or
    ``F.interpolate`` without indices."""
    from padertorch_amd.contrib.je.modules import Pool1d, Pool2d, compute_pad_size, to_pair
    from padertorch_amd.contrib.je.modules.conv_utils import _compute_transpose_out_size
    two = len(plane) == 2
    lengths = [21, 10, 5]
    x0 = np.random.RandomState(8).randn(3, 5, *plane).astype(np.float32)
    pooled, plens, index = (Pool2d if two else Pool1d)('max', size, stride, pad)(torch.from_numpy(x0).cuda(), lengths)
    p = pooled.detach().clone().requires_grad_()
    y, ylens = (mods().Unpool2d if two else mods().Unpool1d)(size, stride, pad)(p, plens, indices=index if with_indices else None)
    pc = pooled.detach().cpu().double().requires_grad_()
    ks, ss = (to_pair(size), to_pair(size if stride is None else stride)) if two else ((size,), (size if stride is None else stride,))
    if with_indices:
        yc = (F.max_unpool2d if two else F.max_unpool1d)(pc, index.cpu(), ks, ss)
        for axis, (k, s, pt) in enumerate(zip(ks, ss, to_pair(pad) if two else (pad,)), 2):
            front, end = compute_pad_size(k, 1, s, pt)
            yc = yc.narrow(axis, front, yc.shape[axis] - front - max(end - s + 1, 0))
    else:
        yc = F.interpolate(pc, scale_factor=ss)
    name = f'unpool {size}/{stride}, pad {pad}, indices {with_indices}'
    close(name + ' y', y, yc.detach(), VALUE)
    assert np.array_equal(ylens, _compute_transpose_out_size(np.asarray(plens), ks[-1], 1, ss[-1], (to_pair(pad) if two else (pad,))[-1]))
    r = torch.from_numpy(np.random.RandomState(9).randn(*yc.shape).astype(np.float32))
    close(name + ' dx', torch.autograd.grad((y * r.cuda()).sum(), p)[0], torch.autograd.grad((yc * r.double()).sum(), pc)[0], GRAD)


def conv64(net, x, lengths, residual=None):
    """A forward (non-transposed) block on ``x [B, C, F, T]``: ``F.pad`` + ``F.conv2d``, then the norm and activation lines."""
    from padertorch_amd.contrib.je.modules import compute_pad_size
    two = net.is_2d()
    kernel, stride, dilation, pad = ((1, v) if not two else v for v in (net.kernel_size, net.stride, net.dilation, net.pad_type))
    (ff, fe), (tf, te) = (compute_pad_size(k, d, s, p) for k, d, s, p in zip(kernel, dilation, stride, pad if two else (None, pad[1])))
    w = net.conv.weight if two else net.conv.weight.unsqueeze(2)
    z = F.conv2d(F.pad(x, (tf, te, ff, fe)), w, net.conv.bias, stride, 0, dilation)
    z = norm_act64(net, z, net.get_output_sequence_lengths(lengths))
    return z if residual is None else z + residual


def autoencoder64(enc, dec, x, lengths):
    """The fixture's pair written out: a ``CNN*d`` of three layers (stride 2 first, batch norm behind the first two, a residual connection
    around the last, a max pool behind it) and its mirror (unpool in front of the first layer, a residual connection around the second,
    stride 2 last; its normalised blocks have ``front = 1``: the quirk); no trim to the target is left."""
    from padertorch_amd.contrib.je.modules.conv_utils import _compute_conv_out_size, _compute_transpose_out_size
    two = x.dim() == 4
    h = conv64(enc.convs[0], x if two else x.unsqueeze(2), lengths)
    lengths = enc.convs[0].get_output_sequence_lengths(lengths)
    h = conv64(enc.convs[2], conv64(enc.convs[1], h, lengths), lengths, h)
    size = (2, 2) if two else (1, 2)
    assert h.shape[2] % size[0] == 0 and h.shape[3] % size[1] == 0          # (the pool pads nothing that stays)
    pooled, index = F.max_pool2d(h, size, return_indices=True)
    lengths = _compute_transpose_out_size(_compute_conv_out_size(lengths, 2, 1, 2, 'both'), 2, 1, 2, 'both')
    d = F.max_unpool2d(pooled, index, size)
    d = block64(dec.convs[1], block64(dec.convs[0], d, lengths), lengths, d)
    d = block64(dec.convs[2], d, lengths)
    return d if two else d.squeeze(2)


def fixture_pair(g, case, dtype=torch.float32):
    """``(maker module, ModuleList([CNN*d, CNNTranspose*d]))`` of a case of ``golden/g28`` from this package's classes and its
    ``get_transpose_config``, the reference's ``state_dict`` loaded strictly."""
    import importlib.util
    import json
    from pathlib import Path
    from padertorch_amd.contrib.je import modules as je
    golden = Path(__file__).resolve().parent / 'golden'
    spec = importlib.util.spec_from_file_location('make_golden_je_conv_transpose', golden / 'make_golden_je_conv_transpose.py')
    mk = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mk)                     # for the seeded inputs and the constructors (the reference is not imported)
    net, mirror = mk.build(case, {'CNN1d': je.CNN1d, 'CNN2d': je.CNN2d}, mods().get_transpose_config, dtype)
    assert mirror == json.loads(str(g[case + '_mirror']))
    net.load_state_dict({k: torch.from_numpy(g[f'{case}_p_{k}']).to(dtype) for k in json.loads(str(g[case + '_keys']))}, strict=True)
    assert json.loads(str(g[case + '_names'])) == [n for n, _ in net.named_parameters()]
    return mk, net


@pytest.mark.parametrize('case', ['t1', 't2'])
def test_autoencoder_against_the_reference(case):
    """The reference's own ``CNN*d`` + mirrored ``CNNTranspose*d`` in fp64 (``golden/g28``): strict load, the mirrored config, the output
    shape and lengths, the pool's indices, values and every gradient - and the same against the fp64 lines above."""
    from test_gpu_je_conv import grad_scale
    g = dict(np.load(Path(__file__).resolve().parent / 'golden' / 'g28_je_conv_transpose.npz', allow_pickle=False))
    mk, pair = fixture_pair(g, case)
    seen = {}

    def run(m, x):
        y, seen['len'], seen['idx'] = mk.call(m, x)
        assert y.shape == x.shape
        return y
    # (check's own r differs from the fixture's: the lines above are held to the kernels with one, the reference with the other)
    check(case + ' lines', pair.cuda(), lambda m, x: autoencoder64(m[0], m[1], x, np.asarray(mk.LENGTHS)), run, mk.inputs(case))
    assert np.array_equal(seen['len'], g[case + '_len']) and np.array_equal(seen['idx'][-1].cpu().numpy(), g[case + '_idx'])
    _, pair = fixture_pair(g, case)
    pair.cuda()
    x = torch.from_numpy(mk.inputs(case)).cuda().requires_grad_()
    y = run(pair, x)
    r = torch.from_numpy(mk.inputs(case, tuple(y.shape))[1]).cuda()
    names = [n for n, _ in pair.named_parameters()]
    grads = torch.autograd.grad((y * r).sum(), [x] + list(pair.parameters()))
    close(case + ' y', y, g[case + '_y64'], VALUE)
    close(case + ' dx', grads[0], g[case + '_g64_x'], GRAD)
    wants = {n: g[f'{case}_g64_{n}'] for n in names}
    for n, got in zip(names, grads[1:]):
        close(f'{case} d {n}', got, wants[n], GRAD, grad_scale(wants, n))


def test_graph_replays_bit_identically():
    """Forward + backward of a gated block without lengths captured in a plain ``torch.cuda.graph``: several replays on new inputs
    against the eager call."""
    torch.manual_seed(7)
    net = perturbed(mods().ConvTranspose2d(8, 16, 3, stride=2, gated=True, activation_fn='tanh'))
    params = list(net.parameters())
    sx = torch.zeros(2, 8, 9, 17).cuda().requires_grad_()
    sr = torch.zeros(*net.get_output_shape(sx.shape).tolist()).cuda()

    def step(x, r):
        y = net(x)[0]
        return [y] + list(torch.autograd.grad((y * r).sum(), [x] + params))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step(sx, sr)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        captured = step(sx, sr)
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


def test_planner_refuses():
    """More taps than the phase table holds: ``NotImplementedError``, not a library call."""
    net = mods().ConvTranspose1d(4, 4, 17, stride=2).cuda()
    with pytest.raises(NotImplementedError, match='taps'):
        net(torch.zeros(1, 4, 8).cuda())
