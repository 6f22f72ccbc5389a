"""The direct 2-D convolution and ``Pool2d`` (``csrc/je_conv2d.hip``) on the paths ``test_gpu_je_conv2d.py`` does not reach: planes around
the 8 x 16 pixel tile, every branch of the planner (a reduced channel chunk, several chunks, a chunk of ``dx`` that holds channels of
both sources, several output-channel tiles), strides and kernels beyond the tested ones, the weight-plane cache across weight updates,
operand scales, pooling with ties / gaps / NaNs / unaligned rows, and what is refused.  The oracle is ``block64`` (``F.pad`` +
``F.conv2d`` in fp64 on the CPU) and, for the max pool, ``max_pool64`` below; the gates are ``test_gpu_je_conv.py``'s, unchanged.
``test_je_conv2d_host.py`` restates the planner and checks that every table entry reaches the path it is named for."""
import copy
import gc

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from test_gpu_je_conv import GRAD, VALUE
from test_gpu_je_conv2d import POOLS, block64, check, close, perturbed

pytestmark = pytest.mark.gpu

B, PLANE = 2, (12, 21)
BASE = (8, 16, 3, {})

#: planes (F, T) around the workgroup tile of 8 x 16 output pixels
EDGES = [(1, 1), (1, 16), (8, 1), (7, 15), (8, 16), (9, 17), (16, 33)]
#: the blocks that also run on the 9 x 17 plane: the tile's edge rows through the epilogue and through the pre-stage
EDGE_BLOCKS = {'gated': dict(gated=True), 'batch norm, pre': dict(norm='batch', activation_fn='relu', pre_activation=True)}

#: one thing at a time away from BASE: (C_in, C_out, kernel, keyword arguments, plane, what the planner must choose: forward / dx launch)
PATHS = {
    'C_in 32, stride 2': (32, 16, 3, dict(stride=2), PLANE, dict(fwd=dict(HF=17, HT=33, CC=16, NCH=2, KS=5))),
    'C_in 32, stride 3': (32, 16, 3, dict(stride=3), PLANE, dict(fwd=dict(HF=24, HT=48, CC=8, NCH=4, KS=3, lds=55296))),
    'C_in 33': (33, 16, 3, {}, PLANE, dict(fwd=dict(Cp=40, CC=32, NCH=2))),
    'gated, C_out 40': (8, 40, 3, dict(gated=True), PLANE, dict(fwd=dict(tiles_n=2), dx=dict(Cp=40, CC=32, NCH=3))),
    'gated, C_out 40, residual': (8, 40, 3, dict(gated=True, residual=True), PLANE, dict(fwd=dict(tiles_n=2), dx=dict(CC=32, NCH=3))),
    'gated, C_out 36': (8, 36, 3, dict(gated=True), PLANE, dict(fwd=dict(tiles_n=2), dx=dict(Cp=40, CC=32, NCH=3))),
    'C_out 64': (8, 64, 3, {}, PLANE, dict(fwd=dict(tiles_n=1), dx=dict(CC=32, NCH=2))),
    'C_out 65': (8, 65, 3, {}, PLANE, dict(fwd=dict(tiles_n=2), dx=dict(Cp=72, CC=32, NCH=3))),
    'kernel 5, stride 2, dilation 2, C_in 32': (32, 16, 5, dict(stride=2, dilation=2), PLANE, dict(fwd=dict(CC=8, NCH=4, KS=7))),
    'kernel (9, 17)': (8, 16, (9, 17), {}, PLANE, dict(fwd=dict(HF=16, HT=32, KS=39), dx=dict(CC=16, KS=77))),
    # the largest halo that keeps a full chunk of 32 channels
    'dilation (4, 6), C_in 32': (32, 16, 3, dict(dilation=(4, 6)), PLANE, dict(fwd=dict(CC=32, NCH=1, lds=64512))),
    'stride (1, 2)': (8, 16, 3, dict(stride=(1, 2)), PLANE, dict(fwd=dict(HF=10, HT=33))),
    'stride (3, 3)': (8, 16, 3, dict(stride=(3, 3)), PLANE, dict(fwd=dict(HF=24, HT=48, CC=8, NCH=1))),
    'stride (2, 3)': (8, 16, 3, dict(stride=(2, 3)), PLANE, dict(fwd=dict(HF=17, HT=48))),
    'kernel 1, stride 2': (8, 16, 1, dict(stride=2), PLANE, dict(fwd=dict(HF=15, HT=31, KS=1), dx=dict(HF=8, HT=16, KS=1))),
    'kernel (2, 2), stride 2, no pad': (8, 16, (2, 2), dict(stride=2, pad_type=None), PLANE, dict(fwd=dict(HF=16, HT=32, KS=1))),
    'stride 2, dilation 2': (8, 16, 3, dict(stride=2, dilation=2), PLANE, dict(fwd=dict(HF=19, HT=35))),
    'stride 2, no pad': (8, 16, 3, dict(stride=(2, 2), pad_type=None), PLANE, dict(fwd=dict(HF=17, HT=33))),
    'stride 2, pad (front, end)': (8, 16, 3, dict(stride=(2, 2), pad_type=('front', 'end')), PLANE, dict(fwd=dict(HF=17, HT=33))),
    'kernel 5': (8, 16, 5, {}, PLANE, dict(fwd=dict(KS=7), dx=dict(CC=16, KS=13))),
    'kernel 5 on 3 x 3': (8, 16, 5, {}, (3, 3), dict(fwd=dict(HF=12, HT=20))),
}
#: the cases in which some input positions are in no window: their dx is exactly zero
UNREACHED = ('kernel 1, stride 2', 'stride 2, no pad', 'kernel (2, 2), stride 2, no pad')

#: refused by the forward planner (the halo of 28 x 52 positions does not fit even with 8 channels); refused by the weight gradient
#: alone (153,856 bytes of LDS) and its widest supported neighbour (94,336 bytes)
REFUSED_FORWARD = (8, 16, 7, dict(stride=3))
REFUSED_WGRAD, WIDEST_WGRAD = (64, 16, 1, dict(stride=2)), (32, 16, 1, dict(stride=2))


def lengths_of(T):
    return [T, max(1, T // 2)]


def make(c_in, c_out, kernel, kwargs, plane, seed=3):
    """``(block on the GPU, x, [residual])`` with seeded weights and input."""
    from padertorch_amd.contrib.je.modules import Conv2d
    kwargs = dict({'activation_fn': 'identity'}, **kwargs)
    has_residual = kwargs.pop('residual', False)
    torch.manual_seed(seed)
    net = perturbed(Conv2d(c_in, c_out, kernel, **kwargs))
    rng = np.random.RandomState(2)
    x0 = rng.randn(B, c_in, *plane).astype(np.float32)
    shape = tuple(int(n) for n in net.get_output_shape(x0.shape))
    return net, x0, [rng.randn(*shape).astype(np.float32)] if has_residual else []


def check_block(name, net, x0, extra=()):
    """``check`` of the block with the lengths of its plane: ``(y, [dx, every parameter gradient])`` of the GPU."""
    lengths = lengths_of(x0.shape[3])
    return check(name, net, lambda m, x, *r: block64(m, x, lengths, *r), lambda m, x, *r: m(x, lengths, _residual=r[0] if r else None)[0],
                 x0, extra)


# ---------------------------------------------------------------------------------------------------------------- plane edges
@pytest.mark.parametrize('plane', EDGES, ids=str)
def test_plane_edges(plane):
    check_block(f'plane {plane}', *make(*BASE, plane))


@pytest.mark.parametrize('name', list(EDGE_BLOCKS))
def test_tile_edge_through_epilogue_and_pre_stage(name):
    check_block(f'plane (9, 17), {name}', *make(8, 16, 3, EDGE_BLOCKS[name], (9, 17)))


# ---------------------------------------------------------------------------------------------------------------- planner paths
def reached(n, k, s, d, front, out):
    """Which of ``n`` input positions some window of ``k`` taps touches."""
    hit = np.zeros(n, bool)
    for o in range(out):
        for tap in range(k):
            p = o * s + tap * d - front
            if 0 <= p < n:
                hit[p] = True
    return hit


@pytest.mark.parametrize('name', list(PATHS))
def test_planner_paths(name):
    from padertorch_amd.contrib.je.modules import compute_pad_size
    c_in, c_out, kernel, kwargs, plane, _ = PATHS[name]
    net, x0, extra = make(c_in, c_out, kernel, kwargs, plane)
    y, got = check_block(name, net, x0, extra)
    if name in UNREACHED:
        hit = [reached(n, k, s, d, compute_pad_size(k, d, s, p)[0], o) for n, k, s, d, p, o in
               zip(plane, net.kernel_size, net.stride, net.dilation, net.pad_type, y.shape[2:])]
        miss_f, miss_t = (torch.from_numpy(~h).cuda() for h in hit)
        assert bool(miss_f.any() or miss_t.any()), name
        dx = got[0]
        assert torch.count_nonzero(dx[:, :, miss_f]) == 0 and torch.count_nonzero(dx[:, :, :, miss_t]) == 0, name
        assert torch.count_nonzero(dx[:, :, ~miss_f][:, :, :, ~miss_t]) > 0


# ---------------------------------------------------------------------------------------------------------------- the weight-plane cache
def test_weight_plane_cache_follows_every_kind_of_weight_update():
    """The packed planes are cached per weight (``ops.je_conv2d._planes_form``).  After each kind of update the values and gradients are
    those of the NEW weights - and the output of the old weights misses the same gate, so a stale plane could not pass."""
    from padertorch_amd.contrib.je.modules import Conv2d
    x0 = np.random.RandomState(2).randn(B, 8, *PLANE).astype(np.float32)
    x = torch.from_numpy(x0).cuda()

    def fresh(seed):
        torch.manual_seed(seed)
        return Conv2d(8, 16, 3, activation_fn='identity').cuda()

    def stale_would_fail(net, y_old):
        with torch.no_grad():
            want = block64(copy.deepcopy(net).cpu().double(), torch.from_numpy(x0).double(), None)
        assert float((y_old.double().cpu() - want).abs().max()) > VALUE * float(want.abs().max())

    net = fresh(20)
    y_old = check('cache, first call', net, lambda m, v: block64(m, v, None), lambda m, v: m(v)[0], x0)[0].detach()
    gen = torch.Generator().manual_seed(21)

    def add_in_place():
        with torch.no_grad():
            for p in net.parameters():
                p.add_((0.1 * torch.randn(p.shape, generator=gen)).cuda())

    def load_state():
        net.load_state_dict({k: v + (0.1 * torch.randn(v.shape, generator=gen)).cuda() for k, v in net.state_dict().items()})

    def assign_data():
        for p in net.parameters():
            p.data = p.data + (0.1 * torch.randn(p.shape, generator=gen)).cuda()

    for change in (add_in_place, load_state, assign_data):
        change()
        stale_would_fail(net, y_old)
        y_old = check(f'cache, {change.__name__}', net, lambda m, v: block64(m, v, None), lambda m, v: m(v)[0], x0)[0].detach()
    for seed in (22, 23, 24):
        # a fresh module where the deleted one was: the same id, version and pointer are all possible
        del net
        gc.collect()
        net = fresh(seed)
        stale_would_fail(net, y_old)
        y_old = check(f'cache, fresh module {seed}', net, lambda m, v: block64(m, v, None), lambda m, v: m(v)[0], x0)[0].detach()
        with torch.no_grad():
            assert torch.equal(net(x)[0], y_old)                                        # and the cached planes give the same bits


# ---------------------------------------------------------------------------------------------------------------- operand scales
def test_zero_input_gives_the_bias_and_no_weight_gradient():
    net, x0, _ = make(*BASE, PLANE)
    y, got = check_block('x = 0', net, np.zeros_like(x0))
    assert torch.equal(y, net.conv.bias.detach()[None, :, None, None].expand_as(y))
    grads = dict(zip([n for n, _ in net.named_parameters()], got[1:]))
    assert torch.count_nonzero(grads['conv.weight']) == 0


def test_zero_upstream_gradient_gives_zero_gradients():
    net, x0, _ = make(*BASE, PLANE)
    x = torch.from_numpy(x0).cuda().requires_grad_()
    y = net(x, lengths_of(PLANE[1]))[0]
    got = torch.autograd.grad((y * torch.zeros_like(y)).sum(), [x] + list(net.parameters()))
    assert len(got) == 3
    for g in got:
        assert bool(torch.isfinite(g).all()) and torch.count_nonzero(g) == 0


@pytest.mark.parametrize('x_scale,w_scale', [(1e4, 1e-3), (1e-4, 1.)])
def test_operands_far_from_unit_scale(x_scale, w_scale):
    net, x0, _ = make(*BASE, PLANE)
    with torch.no_grad():
        net.conv.weight.mul_(w_scale)
    check_block(f'x * {x_scale:g}, W * {w_scale:g}', net, (x0 * x_scale).astype(np.float32))


# ---------------------------------------------------------------------------------------------------------------- Pool2d
def pool_geometry(plane, size, stride, pad):
    """``(front, end, output plane)`` as ``Pool2d`` pads: the pad sizes of a pool whose stride is its size."""
    from padertorch_amd.contrib.je.modules import compute_pad_size, to_pair
    front, end = zip(*[compute_pad_size(k, 1, k, p) for k, p in zip(size, to_pair(pad))])
    return front, end, tuple((n + f + e - k) // s + 1 for n, f, e, k, s in zip(plane, front, end, size, stride))


def max_pool64(x, size, stride, front, end):
    """The rule of ``je_pool2d_forward_kernel`` restated in fp64: zeros in front and behind, trimmed to whole windows; the first of equal
    values in row-major window order; a NaN beats every number.  ``(y, index f T_p + t on the padded and trimmed plane)``."""
    xp = np.pad(x.astype(np.float64), ((0, 0), (0, 0), (front[0], end[0]), (front[1], end[1])))
    OF, OT = ((n - k) // s + 1 for n, k, s in zip(xp.shape[2:], size, stride))
    TP = (OT - 1) * stride[1] + size[1]
    y, index = np.zeros(x.shape[:2] + (OF, OT)), np.zeros(x.shape[:2] + (OF, OT), np.int64)
    for fo in range(OF):
        for to in range(OT):
            best = np.full(x.shape[:2], -np.inf)
            at = np.full(x.shape[:2], fo * stride[0] * TP + to * stride[1], np.int64)
            for a in range(size[0]):
                for w in range(size[1]):
                    pf, pt = fo * stride[0] + a, to * stride[1] + w
                    v = xp[:, :, pf, pt]
                    with np.errstate(invalid='ignore'):
                        take = (v > best) | np.isnan(v)
                    best, at = np.where(take, v, best), np.where(take, pf * TP + pt, at)
            y[:, :, fo, to], index[:, :, fo, to] = best, at
    return y, index


def max_pool64_backward(dy, index, plane, size, stride, front):
    """``dx`` on the input plane: every window's gradient goes to the position its index names (those in the padding are dropped)."""
    Bn, C, OF, OT = dy.shape
    FP, TP = (OF - 1) * stride[0] + size[0], (OT - 1) * stride[1] + size[1]
    flat = np.zeros((Bn, C, FP * TP))
    b, c = np.meshgrid(np.arange(Bn), np.arange(C), indexing='ij')
    np.add.at(flat, (b[..., None, None], c[..., None, None], index), dy.astype(np.float64))
    padded = np.zeros((Bn, C, max(FP, front[0] + plane[0]), max(TP, front[1] + plane[1])))
    padded[:, :, :FP, :TP] = flat.reshape(Bn, C, FP, TP)
    return padded[:, :, front[0]:front[0] + plane[0], front[1]:front[1] + plane[1]]


def check_max_pool(name, x0, size, stride, pad):
    """Values, int64 indices and ``dx`` of ``Pool2d('max', ...)`` against ``max_pool64``: ``(y, index, dx)`` of the GPU."""
    from padertorch_amd.contrib.je.modules import Pool2d, to_pair
    eff = to_pair(size if stride is None else stride)
    front, end, _ = pool_geometry(x0.shape[2:], size, eff, pad)
    yc, ic = max_pool64(x0, size, eff, front, end)
    x = torch.from_numpy(x0).cuda().requires_grad_()
    y, _, index = Pool2d('max', size, stride, pad)(x)
    close(name + ' y', y, yc, VALUE)
    assert index.dtype == torch.int64 and np.array_equal(index.cpu().numpy(), ic), name
    r = np.random.RandomState(9).randn(*yc.shape).astype(np.float32)
    dx = torch.autograd.grad((y * torch.from_numpy(r).cuda()).sum(), x)[0]
    close(name + ' dx', dx, max_pool64_backward(r, ic, x0.shape[2:], size, eff, front), GRAD)
    return y, index, dx


def ties(shape, seed=8):
    """What a pool behind a ReLU sees: half the values zero (as the padding), many equal positives."""
    return np.round(np.maximum(np.random.RandomState(seed).randn(*shape), 0.), 1).astype(np.float32)


@pytest.mark.parametrize('size,stride,pad,C', POOLS)
def test_max_pool_with_ties(size, stride, pad, C):
    x0 = ties((B, C, *PLANE))
    assert (x0 == 0).mean() > .4 and len(np.unique(x0)) < 60
    check_max_pool(f'max pool, ties, {size} / {stride}, pad {pad}, C {C}', x0, size, stride, pad)


@pytest.mark.parametrize('plane,size,stride,pad', [(PLANE, (2, 2), (3, 3), None), (PLANE, (2, 2), (3, 3), 'both'), (PLANE, (3, 3), (1, 1), 'both'),
                                                   ((1, 2), (1, 2), None, None), ((2, 1), (2, 1), None, None)])
@pytest.mark.parametrize('C', [5, 8])
def test_max_pool_gaps_overlaps_and_single_windows(plane, size, stride, pad, C):
    x0 = ties((B, C, *plane), seed=10)
    _, _, dx = check_max_pool(f'max pool, plane {plane}, {size} / {stride}, pad {pad}, C {C}', x0, size, stride, pad)
    if stride == (3, 3):
        front, _, out = pool_geometry(plane, size, stride, pad)
        miss_f, miss_t = (torch.from_numpy(~reached(n, k, s, 1, f, o)).cuda() for n, k, s, f, o in zip(plane, size, stride, front, out))
        assert bool(miss_f.any() and miss_t.any())
        assert torch.count_nonzero(dx[:, :, miss_f]) == 0 and torch.count_nonzero(dx[:, :, :, miss_t]) == 0


@pytest.mark.parametrize('pool_type', ['max', 'avg'])
def test_pool_with_gaps_against_torch(pool_type):
    """Stride larger than the window, average pool included, against torch in fp64 (no ties: standard-normal input)."""
    from padertorch_amd.contrib.je.modules import Pool2d
    x0 = np.random.RandomState(8).randn(B, 8, *PLANE).astype(np.float32)
    xc = torch.from_numpy(x0).double().requires_grad_()
    yc = (F.max_pool2d if pool_type == 'max' else F.avg_pool2d)(xc, (2, 2), (3, 3))
    x = torch.from_numpy(x0).cuda().requires_grad_()
    y = Pool2d(pool_type, (2, 2), (3, 3), None)(x)[0]
    close(f'{pool_type} pool (2, 2) / (3, 3) y', y, yc.detach(), VALUE)
    r = torch.from_numpy(np.random.RandomState(9).randn(*yc.shape).astype(np.float32))
    dx = torch.autograd.grad((y * r.cuda()).sum(), x)[0]
    close(f'{pool_type} pool (2, 2) / (3, 3) dx', dx, torch.autograd.grad((yc * r.double()).sum(), xc)[0], GRAD)
    assert torch.count_nonzero(dx[:, :, 2::3]) == 0 and torch.count_nonzero(dx[:, :, :, 2::3]) == 0


@pytest.mark.parametrize('size,stride,pad,C', [((2, 2), None, 'both', 5), ((3, 2), None, None, 8), ((2, 2), (1, 2), ('front', None), 8)])
def test_max_pool_with_nans(size, stride, pad, C):
    rng = np.random.RandomState(12)
    x0 = ties((B, C, *PLANE), seed=11)
    x0[rng.rand(*x0.shape) < .03] = np.nan
    y, _, _ = check_max_pool(f'max pool, NaNs, {size} / {stride}, pad {pad}, C {C}', x0, size, stride, pad)
    assert 0 < int(torch.isnan(y).sum()) < y.numel()


@pytest.mark.parametrize('pool_type', ['max', 'avg'])
@pytest.mark.parametrize('wide,first', [(12, 1), (13, 0)])
def test_pool_of_a_channel_slice_takes_the_scalar_route(pool_type, wide, first):
    """Eight channels (a multiple of four) whose pointer (12 channels, from the second) or row stride (13 channels) is no multiple of 16
    bytes: the bits of the contiguous copy, which takes the vector route."""
    from padertorch_amd.contrib.je.modules import Pool2d
    rows = torch.from_numpy(ties((B, *PLANE, wide), seed=13)).cuda()
    view = rows.permute(0, 3, 1, 2)[:, first:first + 8]
    assert view.stride(1) == 1 and (view.data_ptr() % 16 != 0 or (4 * view.stride(3)) % 16 != 0)
    pool = Pool2d(pool_type, (2, 2), None, 'both')
    out = []
    for x in (view.detach().requires_grad_(), view.contiguous().requires_grad_()):
        y, _, index = pool(x)
        r = torch.from_numpy(np.random.RandomState(9).randn(*y.shape).astype(np.float32)).cuda()
        out.append((y, index, torch.autograd.grad((y * r).sum(), x)[0]))
    for a, b in zip(*out):
        assert (a is None and b is None) or torch.equal(a, b)
    assert (out[0][1] is not None) == (pool_type == 'max')


# ---------------------------------------------------------------------------------------------------------------- refusals
def test_forward_refusal_comes_from_the_first_call():
    from padertorch_amd.contrib.je.modules import Conv2d
    c_in, c_out, kernel, kwargs = REFUSED_FORWARD
    net = Conv2d(c_in, c_out, kernel, **kwargs).cuda()
    with pytest.raises(NotImplementedError, match='halo'):
        net(torch.zeros(B, c_in, *PLANE).cuda())


def test_weight_gradient_refusal_comes_from_the_forward_call():
    """A layer whose weight gradient is not built: the forward of a trainable layer says so and names the geometry; without a weight
    that requires a gradient the layer runs, ``dx`` included.  Its widest supported neighbour passes every gate."""
    check_block('kernel 1, stride 2, C_in 32', *make(*WIDEST_WGRAD, PLANE))
    net, x0, _ = make(*REFUSED_WGRAD, PLANE)
    x = torch.from_numpy(x0).cuda()
    lengths = lengths_of(PLANE[1])
    with pytest.raises(NotImplementedError, match=r'weight gradient.*\[2, 12, 21, 64, 6, 11, 16, 1, 1, 1, 2, 2, 1, 1, 0, 0\]'):
        net(x, lengths)
    want = block64(copy.deepcopy(net).cpu().double(), torch.from_numpy(x0).double().requires_grad_(), lengths)
    with torch.no_grad():
        close('kernel 1, stride 2, C_in 64, no_grad y', net(x, lengths)[0], want.detach(), VALUE)
    net.freeze()
    xg = x.clone().requires_grad_()
    y = net(xg, lengths)[0]
    r = torch.from_numpy(np.random.RandomState(5).randn(*y.shape).astype(np.float32))
    close('kernel 1, stride 2, C_in 64, frozen y', y, want.detach(), VALUE)
    xc = torch.from_numpy(x0).double().requires_grad_()
    wc = block64(copy.deepcopy(net).cpu().double(), xc, lengths)
    close('kernel 1, stride 2, C_in 64, frozen dx', torch.autograd.grad((y * r.cuda()).sum(), xg)[0],
          torch.autograd.grad((wc * r.double()).sum(), xc)[0], GRAD)
