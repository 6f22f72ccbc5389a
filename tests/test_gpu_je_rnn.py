"""contrib/je's RNN wrappers, the GRU recurrence kernels and the sequence poolings on the GPU against the reference's fp64 run
(tests/golden/g25_je_rnn.npz) or the fp64 restatement tests/je_rnn_ref.py on the same inputs.

Gates: values |diff| <= 1e-5 max|want|, gradients <= 2e-4 max|want|; the reference's own fp32 run stays within 0.015 of them on the
fixture (make_golden_je_rnn.py prints the shares).  Every comparison prints its ratio diff / (gate max|want|) (run with -s;
profiles/je_rnn_gates.txt is that output).

The reference's ``NaN * 0``: ``reverse_sequence`` reproduces it (a NaN behind the length stays NaN where the reference's wrapped gather
reads it); ``Sum``, ``Mean`` and ``AutoPool`` depart from it: the kernels never read behind the length, so a NaN there does not reach the
result (the reference's mask multiply would make the whole row's result NaN).
"""
import importlib.util
import json
from pathlib import Path

import numpy as np
import pytest
import torch

import je_rnn_ref as ref

pytestmark = pytest.mark.gpu

GOLDEN = Path(__file__).resolve().parent / 'golden'
VALUE, GRAD = 1e-5, 2e-4
MODES = {'Sum': 'sum', 'Mean': 'mean', 'Max': 'max', 'TakeLast': 'last'}


@pytest.fixture(scope='module')
def g25():
    d = dict(np.load(GOLDEN / 'g25_je_rnn.npz', allow_pickle=False))
    spec = importlib.util.spec_from_file_location('make_golden_je_rnn', GOLDEN / 'make_golden_je_rnn.py')
    d['maker'] = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(d['maker'])             # for the seeded inputs (the reference is not imported)
    return d


def close(name, got, want, gate, scale=None):
    got = got.detach().double().cpu().reshape(-1)
    want = torch.as_tensor(want).detach().double().reshape(-1)
    assert got.shape == want.shape, (name, got.shape, want.shape)
    finite = torch.isfinite(want)
    assert torch.equal(torch.isfinite(got), finite) and torch.equal(got[~finite].nan_to_num(7., 8., 9.), want[~finite].nan_to_num(7., 8., 9.)), name
    got, want = got[finite], want[finite]
    if scale is None:
        scale = float(want.abs().max()) if want.numel() else 0.
    err = float((got - want).abs().max()) if want.numel() else 0.
    ratio = err / (gate * scale) if scale > 0 else (0. if err == 0 else float('inf'))
    print(f'{name}: {ratio:.3f} of the gate ({err:.2e} against max {scale:.2e})')
    assert ratio <= 1., (name, ratio)


def noncontiguous(x0):
    """The array on the GPU as a view with gaps in its last axis."""
    wide = torch.zeros(*x0.shape[:-1], x0.shape[-1] + 3).cuda()
    wide[..., 1:-2] = torch.from_numpy(np.ascontiguousarray(x0)).cuda()
    x = wide[..., 1:-2]
    assert not x.is_contiguous()
    return x


# ---------------------------------------------------------------------------------------------------- the fixture through the modules
def build(g, case):
    from padertorch_amd.contrib.je import modules as je
    mk = g['maker']
    kind, H, layers, bidir, bias, reverse, _ = mk.RNN_CASES[case]
    if kind == 'transformer':
        net = je.TransformerEncoder(je.TransformerLayerStack(mk.F, H, num_layers=layers, **mk.TRANSFORMER), reverse=reverse)
    else:
        cls = torch.nn.LSTM if kind == 'lstm' else torch.nn.GRU
        net = (je.LSTM if kind == 'lstm' else je.GRU)(cls(mk.F, H, layers, bias=bias, batch_first=True, bidirectional=bidir), reverse=reverse)
    nets = torch.nn.ModuleDict(dict(rnn=net))
    if kind == 'gru+autopool':
        nets['pool'] = je.AutoPool(mk.out_channels(case), alpha=mk.ALPHA, trainable=True)
    keys = json.loads(str(g[case + '_keys']))
    nets.load_state_dict({k: torch.from_numpy(g[f'{case}_p_{k}']) for k in keys}, strict=True)
    return nets.cuda()


def run(nets, x, r, lengths):
    x = x.detach().requires_grad_()
    y, _ = nets['rnn'](x, lengths)
    if 'pool' in nets:
        y = nets['pool'](y, lengths)
    grads = torch.autograd.grad((y * r).sum(), [x] + list(nets.parameters()))
    return [y.detach()] + list(grads)


def check(g, case, tag, res, names, flip=False):
    mk = g['maker']
    close(f'{case} y{tag}', res[0].flip(0) if flip else res[0], g[case + '_y64'], VALUE)
    close(f'{case} dx{tag}', res[1].flip(0) if flip else res[1], g[case + '_g64_x'], GRAD)
    for n, got in zip(names, res[2:]):
        want = g[f'{case}_g64_{n}']
        if np.abs(want).max() < mk.ZERO:
            # analytically zero (a key bias under the softmax): no scale of its own; it is a sum of the same terms as the query bias's
            # gradient of the same attention, whose size is the scale the gate is taken of
            assert n.endswith('lin_key.bias'), n
            scale = float(np.abs(g[f'{case}_g64_{n.replace("lin_key", "lin_queue")}']).max())
            close(f'{case} d {n}{tag} (zero; scale of lin_queue.bias)', got, want, GRAD, scale)
        else:
            close(f'{case} d {n}{tag}', got, want, GRAD)


@pytest.mark.parametrize('case', ['r0', 'r1', 'r2', 'r3', 'r4'])
def test_fixture_cases(g25, case):
    mk = g25['maker']
    nets = build(g25, case)
    x0, r0 = mk.rnn_inputs(case)
    x, r = noncontiguous(x0), torch.from_numpy(r0).cuda()
    lengths = mk.RNN_CASES[case][6]
    names = json.loads(str(g25[case + '_names']))
    assert names == [n for n, _ in nets.named_parameters()]
    res = run(nets, x, r, lengths)
    check(g25, case, '', res, names)
    if lengths is None:
        return
    if 'pool' not in nets:
        for b, n in enumerate(lengths):                 # zero behind each length, as pad_packed_sequence gives
            assert torch.all(res[0][b, :, n:] == 0)
    for form in (torch.tensor(lengths), torch.tensor(lengths, device='cuda'), torch.tensor(lengths, device='cuda', dtype=torch.int32),
                 np.asarray(lengths)):
        for a, b in zip(res, run(nets, x, r, form)):
            assert torch.equal(a, b)
    # ascending lengths: the batch reversed gives the reversed results (pack_padded_sequence would refuse it)
    check(g25, case, ', batch reversed', run(nets, x.flip(0), r.flip(0), lengths[::-1]), names, flip=True)


def test_fixture_poolings(g25):
    from padertorch_amd.contrib.je.modules import reduce
    mk = g25['maker']
    for key, name, wl, axis, keep in mk.pool_cases():
        module = getattr(reduce, name)(axis=axis, keepdims=keep)
        x = noncontiguous(mk.pool_inputs(key)).requires_grad_()
        out = module(x, list(mk.LENGTHS) if wl else None)
        if name == 'Max':
            assert out[1].dtype == torch.int64 and torch.equal(out[1].cpu(), torch.from_numpy(g25[key + '_idx'])), key
            out = out[0]
        assert tuple(out.shape) == g25[key + '_y64'].shape, key
        close(key, out, g25[key + '_y64'], VALUE)
        _, r = mk.pool_inputs(key, tuple(out.shape))
        close(key + ' dx', torch.autograd.grad((out * torch.from_numpy(r).cuda()).sum(), x)[0], g25[key + '_g64_x'], GRAD)


def test_fixture_autopool_and_reverse(g25):
    from padertorch_amd.contrib.je.modules import reduce, rnn
    mk = g25['maker']
    for trainable in 'tf':
        for wl in 'ln':
            key = f'a_{trainable}_{wl}'
            pool = reduce.AutoPool(mk.F, alpha=mk.ALPHA, trainable=trainable == 't').cuda()
            x = noncontiguous(mk.pool_inputs(key)).requires_grad_()
            out = pool(x, list(mk.LENGTHS) if wl == 'l' else None)
            close(key, out, g25[key + '_y64'], VALUE)
            _, r = mk.pool_inputs(key, tuple(out.shape))
            grads = torch.autograd.grad((out * torch.from_numpy(r).cuda()).sum(), [x] + list(pool.parameters()))
            close(key + ' dx', grads[0], g25[key + '_g64_x'], GRAD)
            if trainable == 't':
                assert grads[1].shape == (mk.F, 1)
                close(key + ' dalpha', grads[1], g25[key + '_g64_alpha'], GRAD)
    for wl in 'ln':
        key = f'v_{wl}'
        x = noncontiguous(mk.pool_inputs(key)).requires_grad_()
        out = rnn.reverse_sequence(x, list(mk.LENGTHS) if wl == 'l' else None)
        assert torch.equal(out.cpu(), torch.from_numpy(g25[key + '_y32'])), key          # a gather: exact
        _, r = mk.pool_inputs(key, tuple(out.shape))
        assert torch.equal(torch.autograd.grad((out * torch.from_numpy(r).cuda()).sum(), x)[0].cpu(), torch.from_numpy(g25[key + '_g32_x']))


# ---------------------------------------------------------------------------------------------------- chunk_gru alone
def _table(nseq, T, stride, counts):
    """``nseq`` sequences of room ``T``: stride 1: one after the other; stride > 1: interleaved in groups of ``stride`` (``nseq`` a multiple
    of it: every row belongs to a sequence, as the weight-gradient GEMMs behind the kernel require)."""
    assert stride == 1 or nseq % stride == 0
    rows = []
    for i in range(nseq):
        base = i * T if stride == 1 else (i // stride) * stride * T + i % stride
        rows.append([base, stride, counts[i % len(counts)]])
    return torch.tensor(rows, dtype=torch.int32), nseq * T


# H: 4, 5, 20, 40, 128 resident (HP 32, 32, 32, 64, 128); 130, 160 streamed; 832 streamed with 80 * 832 = 66560 bytes of dynamic LDS in
# the backward kernel, above the default 64 KB.  Sequence counts 1, 3, 4, 5, 9; T 1..7; stride 1 and 3; N != H.
@pytest.mark.parametrize('nseq,T,stride,H,N,bi,bias,flip', [
    (1, 1, 1, 4, 3, True, True, False), (3, 2, 1, 5, 7, True, True, True), (4, 7, 1, 20, 6, True, False, False),
    (3, 6, 3, 20, 9, False, True, True), (5, 5, 1, 40, 8, True, True, False), (9, 3, 3, 128, 16, True, True, True),
    (5, 4, 1, 128, 64, False, False, False), (4, 3, 1, 64, 5, True, True, True), (5, 4, 1, 160, 12, True, True, False),
    (3, 3, 3, 130, 6, False, True, True), (9, 2, 1, 130, 4, True, False, True), (2, 2, 1, 832, 4, False, True, False)])
def test_chunk_gru_against_restatement(nseq, T, stride, H, N, bi, bias, flip):
    from padertorch_amd.ops import gru
    torch.manual_seed(nseq * 100 + H)
    counts = [T, 0, 1, T, T - 1 if T > 1 else 1]                # 0, 1 and T mixed inside one tile of four
    table, rows = _table(nseq, T, stride, counts)
    rnn = torch.nn.GRU(N, H, bias=bias, bidirectional=bi, batch_first=True).cuda()
    D = 2 if bi else 1
    names = [n for n, _ in rnn.named_parameters()]
    per = 4 if bias else 2
    slots = []
    for d in range(D):
        p = list(rnn.parameters())[d * per:(d + 1) * per]
        slots += p + [None] * (4 - per)
    slots += [None] * (8 - len(slots))
    x = torch.randn(rows, N).cuda().requires_grad_()
    r = torch.randn(rows, D * H)
    h = gru.chunk_gru(x, table.cuda(), T, *slots, flip=flip)
    grads = torch.autograd.grad((h * r.cuda()).sum(), [x] + list(rnn.parameters()))
    ps = [p.detach().double().cpu().requires_grad_() for p in rnn.parameters()]
    dirs = [tuple(ps[d * per:(d + 1) * per]) + (None,) * (4 - per) for d in range(D)]
    xr = x.detach().double().cpu().requires_grad_()
    want = ref.gru_layer(xr, table.tolist(), T, dirs, flip=flip)
    want_grads = torch.autograd.grad((want * r.double()).sum(), [xr] + ps)
    close('h', h, want, VALUE)
    on_step = torch.zeros(rows, dtype=torch.bool)
    for b, s, n in table.tolist():
        on_step[[b + t * s for t in range(n)]] = True
    assert torch.all(h[(~on_step).cuda()] == 0)                 # exactly zero on the rows of no step
    close('dx', grads[0], want_grads[0], GRAD)
    for n, g, w in zip(names, grads[1:], want_grads[1:]):
        close('d ' + n, g, w, GRAD)


def test_chunk_gru_skips_a_sequence_outside_the_buffer_and_runs_backward_once():
    from padertorch_amd.ops import gru
    torch.manual_seed(3)
    rnn = torch.nn.GRU(3, 4, batch_first=True).cuda()
    x = torch.randn(8, 3).cuda().requires_grad_()
    good = torch.tensor([[0, 1, 4], [4, 1, 3]], dtype=torch.int32).cuda()
    bad = torch.tensor([[0, 1, 4], [4, 1, 3], [6, 1, 4], [-1, 1, 2]], dtype=torch.int32).cuda()       # rows 6..9 and -1..2: not inside
    params = list(rnn.parameters()) + [None] * 4
    h = gru.chunk_gru(x, good, 4, *params)
    assert torch.equal(h, gru.chunk_gru(x, bad, 4, *params))
    loss = h.sum()
    loss.backward(retain_graph=True)
    with pytest.raises(RuntimeError, match='runs once per forward'):
        loss.backward()


# ---------------------------------------------------------------------------------------------------- seq_pool and reverse_sequence alone
def _pool_lengths(T, mode):
    if mode in ('sum', 'mean', 'max'):
        return [T, 1, 0, max(1, T // 2)]
    return [T, 1, max(1, T - 1), max(1, T // 2)]


@pytest.mark.parametrize('T', [1, 63, 64, 65, 257])
@pytest.mark.parametrize('layout', ['bct', 'btc'])
def test_seq_pool_against_restatement(T, layout):
    """``bct``: time contiguous, a wavefront per row; ``btc``: time strided, a thread per column.  Inner sizes 1, 3, 10; lengths 1, T and
    (sum, mean, max) 0; inputs are views with gaps; continuous draws, so no ties for ``max``."""
    from padertorch_amd.ops.seq_pool import seq_pool
    rng = np.random.RandomState(T)
    for C in (1, 3, 10):
        x0 = rng.randn(*((4, C, T) if layout == 'bct' else (4, T, C))).astype(np.float32)
        axis = -1 if layout == 'bct' else 1
        for mode in ('sum', 'mean', 'max', 'last', 'autopool'):
            for with_lengths in (True, False):
                lengths = _pool_lengths(T, mode) if with_lengths else None
                x, ax, alpha = noncontiguous(x0), axis, None
                if mode == 'autopool':                  # [B, C, T] along the last axis: as it is, or the transposed view (time strided)
                    x, ax, alpha = (x if layout == 'bct' else x.transpose(1, 2)), -1, torch.linspace(0.5, 2., C)[:, None]
                x = x.detach().requires_grad_()
                xr = x.detach().double().cpu().requires_grad_()
                a_gpu = None if alpha is None else alpha.cuda().requires_grad_()
                a_ref = None if alpha is None else alpha.double().requires_grad_()
                got = seq_pool(x, lengths, ax, mode, False, alpha=a_gpu)
                want = ref.seq_pool(xr, lengths, ax, mode, False, alpha=a_ref)
                tag = f'{layout} T={T} C={C} {mode} {"ragged" if with_lengths else "full"}'
                if mode == 'max':
                    assert torch.equal(got[1].cpu(), want[1]), tag
                    got, want = got[0], want[0]
                if with_lengths and mode in ('sum', 'mean', 'max'):
                    assert torch.all(got[2] == (-np.inf if mode == 'max' else 0.)), tag          # length 0
                close(tag, got, want, VALUE)
                r = torch.from_numpy(rng.randn(*want.shape))
                fin = torch.isfinite(want)
                gg = torch.autograd.grad((got[fin.cuda()] * r[fin].float().cuda()).sum(), [x] + ([a_gpu] if alpha is not None else []))
                gw = torch.autograd.grad((want[fin] * r[fin].float().double()).sum(), [xr] + ([a_ref] if alpha is not None else []))
                close(tag + ' dx', gg[0], gw[0], GRAD)
                if alpha is not None:
                    close(tag + ' dalpha', gg[1], gw[1], GRAD)


def test_seq_pool_four_dimensions_and_keepdims():
    from padertorch_amd.ops.seq_pool import seq_pool
    rng = np.random.RandomState(4)
    x0 = rng.randn(3, 2, 5, 65).astype(np.float32)              # [B, C, F, T]
    lengths = [65, 1, 0]
    for x in (noncontiguous(x0), torch.from_numpy(x0).cuda()[:, :, ::3]):          # (C, F) collapse / do not collapse (one copy)
        for mode in ('sum', 'mean'):
            for axis in (-1, 2):
                xg = x.detach().requires_grad_()
                xr = x.detach().double().cpu().requires_grad_()
                got, want = seq_pool(xg, lengths, axis, mode, True), ref.seq_pool(xr, lengths, axis, mode, True)
                assert got.shape == want.shape
                close(f'4-D {mode} axis {axis}', got, want, VALUE)
                r = torch.from_numpy(rng.randn(*want.shape))
                close(f'4-D {mode} axis {axis} dx', torch.autograd.grad((got * r.float().cuda()).sum(), xg)[0],
                      torch.autograd.grad((want * r.float().double()).sum(), xr)[0], GRAD)
    x = torch.from_numpy(x0).cuda()
    last = seq_pool(x, [65, 1, 7], 3, 'last', True)
    assert last.shape == (3, 2, 5, 1) and torch.equal(last[..., 0], torch.stack([x[0, ..., 64], x[1, ..., 0], x[2, ..., 6]]))
    assert torch.equal(seq_pool(x, None, 2, 'last'), x[:, :, -1])


@pytest.mark.parametrize('T', [1, 63, 64, 65, 257])
def test_reverse_sequence_against_restatement(T):
    from padertorch_amd.ops.seq_pool import reverse_sequence
    rng = np.random.RandomState(T)
    for C in (1, 3, 10):
        x0 = rng.randn(4, T, C).astype(np.float32)
        for lengths in ([T, 1, max(1, T // 2), max(1, T - 1)], None):
            for x in (noncontiguous(x0), torch.from_numpy(np.ascontiguousarray(x0.transpose(0, 2, 1))).cuda().transpose(1, 2)):
                x = x.detach().requires_grad_()
                xr = x.detach().double().cpu().requires_grad_()
                got, want = reverse_sequence(x, lengths), ref.reverse_sequence(xr, lengths)
                assert got.is_contiguous() and torch.equal(got.double().cpu(), want)
                r = torch.from_numpy(rng.randn(4, T, C))
                assert torch.equal(torch.autograd.grad((got * r.float().cuda()).sum(), x)[0].double().cpu(),
                                   torch.autograd.grad((want * r.float().double()).sum(), xr)[0])


def test_nan_behind_the_length():
    """``reverse_sequence``: the reference's ``x[(len - 1 - t) mod T] * 0`` behind the length keeps a NaN it reads - reproduced.  ``Sum``,
    ``Mean``, ``AutoPool``: the reference's ``x * mask`` would turn the row's result into NaN; the kernels never read behind the length -
    a documented departure.  The backward of ``reverse_sequence`` writes plain zeros behind the length."""
    from padertorch_amd.ops.seq_pool import reverse_sequence, seq_pool
    x = torch.ones(1, 4, 2).cuda()
    x[0, 3] = float('nan')
    out = reverse_sequence(x, [2])
    assert torch.isnan(out[0, 2]).all() and torch.all(out[0, 3] == 0) and torch.all(out[0, :2] == 1)
    g = torch.full((1, 4, 2), float('nan')).cuda()
    g[0, :2] = 1.
    xg = torch.ones(1, 4, 2).cuda().requires_grad_()
    assert torch.equal(torch.autograd.grad(reverse_sequence(xg, [2]), xg, g)[0], torch.tensor([[[1., 1.], [1., 1.], [0., 0.], [0., 0.]]]).cuda())
    for layout in ('bct', 'btc'):
        if layout == 'bct':
            xp, axis = torch.ones(2, 3, 5).cuda(), -1
            xp[:, :, 3:] = float('nan')
        else:
            xp, axis = torch.ones(2, 5, 3).cuda(), 1
            xp[:, 3:] = float('nan')
        assert torch.all(seq_pool(xp, [3, 2], axis, 'sum') == torch.tensor([3., 2.]).cuda()[:, None])
        assert torch.allclose(seq_pool(xp, [3, 2], axis, 'mean'), torch.ones(()).cuda())
        assert torch.all(seq_pool(xp, [3, 2], axis, 'max')[0] == 1)
        if layout == 'bct':
            assert torch.allclose(seq_pool(xp, [3, 2], axis, 'autopool', alpha=1.), torch.ones(()).cuda())
        assert torch.isnan(seq_pool(xp, [5, 4], axis, 'sum')).all()                       # inside the length a NaN counts


# ---------------------------------------------------------------------------------------------------- capture
def test_capture_replays_equal_eager_bit_for_bit(g25):
    from padertorch_amd.ops import capture
    mk = g25['maker']
    nets = build(g25, 'r4')
    x0, r0 = mk.rnn_inputs('r4')
    x, r = torch.from_numpy(x0).cuda(), torch.from_numpy(r0).cuda()
    lengths = torch.tensor(mk.LENGTHS, device='cuda')
    run(nets, x, r, lengths)                                             # warm-up: every cache is filled
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode('error')
    try:
        first = run(nets, x, r, lengths)                                 # no .item() / .cpu() on the way
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    sx, sr, sl = x.clone(), r.clone(), lengths.clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        run(nets, sx, sr, sl)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with capture.capture_mode():
        with torch.cuda.graph(graph, stream=side):
            capture.zero_block(sx.device)
            captured = run(nets, sx, sr, sl)
    graph.replay()
    torch.cuda.synchronize()
    for k, (a, b) in enumerate(zip(captured, first)):
        assert torch.equal(a, b), ('replay', k)
    for pattern in ([3, 19, 7, 12], [19, 19, 1, 2]):
        other = torch.tensor(pattern, device='cuda')
        sl.copy_(other)
        graph.replay()
        torch.cuda.synchronize()
        eager = run(nets, x, r, other)
        assert not torch.equal(eager[0], first[0])
        for k, (a, b) in enumerate(zip(captured, eager)):
            assert torch.equal(a, b), ('replay', pattern, k)
