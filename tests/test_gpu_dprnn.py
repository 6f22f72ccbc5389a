"""DPRNN and its kernels (csrc/dprnn.hip) against the reference's fp64 results (tests/golden/g17_dprnn.npz) and fp64 restatements with
torch's own operators on the CPU.

Gates (those of tests/test_gpu_convnet.py): values |diff| <= 1e-5 max|want|, gradients |diff| <= 2e-4 max|want|.  The reference's own
fp32 run stays within 0.016 / 0.005 of them on the fixture (make_golden_dprnn.py prints the shares).  Every comparison prints its ratio
diff / (gate max|want|) (run with -s).

chunk_lstm shapes: the recurrence kernel owns TILE = 4 sequences per workgroup and pads H to 32 / 64 / 128, so the sequence counts are
1, 3, 4, 5 and 9 (a third workgroup), H is 4, 5, 20 (padded to 32), 40 (64), 128 and 130 / 160 / 512 / 1100 (W_hh streamed; 1100 needs more than the default 64 KB of dynamic LDS), T is 1 to 7, the step stride 1 and 3, the
counts 0, 1 and T mixed inside one tile."""
import importlib.util
import json
from pathlib import Path

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GOLDEN = Path(__file__).resolve().parent / 'golden'
VALUE, GRAD = 1e-5, 2e-4


@pytest.fixture(scope='module')
def g17():
    d = dict(np.load(GOLDEN / 'g17_dprnn.npz', allow_pickle=False))
    d['cases'] = json.loads(str(d['cases']))
    d['tasnet'] = json.loads(str(d['tasnet']))
    spec = importlib.util.spec_from_file_location('make_golden_dprnn', GOLDEN / 'make_golden_dprnn.py')
    d['maker'] = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(d['maker'])             # for inputs(): the seeded x and r (the reference is not imported)
    return d


def close(name, got, want, gate):
    got = got.detach().double().cpu().reshape(-1)
    want = torch.as_tensor(want).double().reshape(-1)
    assert got.shape == want.shape, (name, got.shape, want.shape)
    scale = float(want.abs().max())
    err = float((got - want).abs().max())
    ratio = err / (gate * scale) if scale > 0 else (0. if err == 0 else float('inf'))
    print(f'{name}: {ratio:.3f} of the gate ({err:.2e} against max {scale:.2e})')
    assert ratio <= 1., (name, ratio)


def build(g, i):
    from padertorch_amd.modules import DPRNN
    N, H, K, P, blocks, intra, inter, B, L, lengths = g['cases'][i]
    net = DPRNN(N, H, K, P, blocks, inter_chunk_type=inter, intra_chunk_type=intra)
    keys = json.loads(str(g[f'c{i}_keys']))
    net.load_state_dict({k: torch.from_numpy(g[f'c{i}_p_{k}']) for k in keys}, strict=True)
    return net.cuda()


def run(net, x, r, lengths):
    x = x.detach().requires_grad_()
    y = net(x, lengths)
    grads = torch.autograd.grad((y * r).sum(), [x] + list(net.parameters()))
    return [y.detach()] + list(grads)


@pytest.mark.parametrize('i', [0, 1, 2, 3])
def test_fixture_cases(g17, i):
    case = g17['cases'][i]
    net = build(g17, i)
    x0, r0 = g17['maker'].inputs(case, int(g17[f'c{i}_seed']))
    wide = torch.zeros(x0.shape[0], x0.shape[1], x0.shape[2] + 3).cuda()
    wide[..., 1:-2] = torch.from_numpy(x0).cuda()
    x = wide[..., 1:-2]                                                  # a non-contiguous view
    assert not x.is_contiguous()
    r = torch.from_numpy(r0).cuda()
    lengths = case[9]
    res = run(net, x, r, lengths)
    names = json.loads(str(g17[f'c{i}_names']))
    assert names == [n for n, _ in net.named_parameters()]
    close(f'c{i} y', res[0], g17[f'c{i}_y64'], VALUE)
    close(f'c{i} dx', res[1], g17[f'c{i}_g64_x'], GRAD)
    for n, g in zip(names, res[2:]):
        close(f'c{i} d {n}', g, g17[f'c{i}_g64_{n}'], GRAD)
    if lengths is None:
        return
    for form in (torch.tensor(lengths), torch.tensor(lengths, device='cuda'), torch.tensor(lengths, device='cuda', dtype=torch.int32)):
        for a, b in zip(res, run(net, x, r, form)):
            assert torch.equal(a, b)
    # ascending lengths: the batch reversed gives the reversed results (pack_padded_sequence would refuse it)
    flipped = run(net, x.flip(0), r.flip(0), lengths[::-1])
    close(f'c{i} y, batch reversed', flipped[0].flip(0), g17[f'c{i}_y64'], VALUE)
    close(f'c{i} dx, batch reversed', flipped[1].flip(0), g17[f'c{i}_g64_x'], GRAD)
    for n, g in zip(names, flipped[2:]):
        close(f'c{i} d {n}, batch reversed', g, g17[f'c{i}_g64_{n}'], GRAD)


def _tasnet(g):
    from padertorch_amd.contrib.examples.source_separation.tasnet.model import TasNet
    from padertorch_amd.contrib.examples.source_separation.tasnet.tas_coders import TasDecoder, TasEncoder
    from padertorch_amd.modules import DPRNN
    c, i = g['tasnet'], len(g['cases'])
    net = TasNet(TasEncoder(c['L'], c['N']), DPRNN(c['N'], c['rnn_size'], c['window'], c['hop'], c['blocks']), TasDecoder(c['L'], c['N']),
                 num_speakers=c['K'])
    keys = json.loads(str(g[f'c{i}_keys']))
    net.load_state_dict({k: torch.from_numpy(g[f'c{i}_p_{k}']) for k in keys}, strict=True)
    return net.cuda(), c, i


def _tasnet_step(net, y, r, lengths):
    y = y.detach().requires_grad_()
    out = net(dict(y=y, num_samples=lengths))['out']
    grads = torch.autograd.grad((out * r).sum(), [y] + list(net.parameters()))
    return [out.detach()] + list(grads)


def test_tasnet_with_dprnn(g17):
    net, c, i = _tasnet(g17)
    y0, r0 = g17['maker'].tasnet_inputs(int(g17[f'c{i}_seed']))
    res = _tasnet_step(net, torch.from_numpy(y0).cuda(), torch.from_numpy(r0).cuda(), list(c['num_samples']))
    names = json.loads(str(g17[f'c{i}_names']))
    close('tasnet out', res[0], g17[f'c{i}_y64'], VALUE)
    close('tasnet d y', res[1], g17[f'c{i}_g64_x'], GRAD)
    for n, g in zip(names, res[2:]):
        close(f'tasnet d {n}', g, g17[f'c{i}_g64_{n}'], GRAD)


def test_capture_replays_equal_eager_bit_for_bit(g17):
    from padertorch_amd.ops import capture
    net, c, i = _tasnet(g17)
    y0, r0 = g17['maker'].tasnet_inputs(int(g17[f'c{i}_seed']))
    y, r = torch.from_numpy(y0).cuda(), torch.from_numpy(r0).cuda()
    lengths = torch.tensor(c['num_samples'], device='cuda')
    _tasnet_step(net, y, r, lengths)                                      # warm-up: every cache is filled
    mode = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode('error')
    try:
        first = _tasnet_step(net, y, r, lengths)                          # no .item() / .cpu() on the way
    finally:
        torch.cuda.set_sync_debug_mode(mode)
    sy, sr, sl = y.clone(), r.clone(), lengths.clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        _tasnet_step(net, sy, sr, sl)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with capture.capture_mode():
        with torch.cuda.graph(graph, stream=side):
            capture.zero_block(sy.device)
            captured = _tasnet_step(net, sy, sr, sl)
    graph.replay()
    torch.cuda.synchronize()
    for k, (a, b) in enumerate(zip(captured, first)):
        assert torch.equal(a, b), ('replay', k)
    for pattern in ([30, 62], [62, 7]):
        other = torch.tensor(pattern, device='cuda')
        sl.copy_(other)
        graph.replay()
        torch.cuda.synchronize()
        eager = _tasnet_step(net, y, r, other)
        assert not torch.equal(eager[0], first[0])
        for k, (a, b) in enumerate(zip(captured, eager)):
            assert torch.equal(a, b), ('replay', pattern, k)


# ---------------------------------------------------------------------------------------------------- chunk_lstm alone
def _lstm_reference(rnn, x, table, cap):
    """fp64 on the CPU: every sequence of the table through ``rnn`` over ``pack_padded_sequence``; zeros on the rows off the steps."""
    from torch.nn.utils.rnn import pack_padded_sequence, pad_packed_sequence
    ref = torch.nn.LSTM(rnn.input_size, rnn.hidden_size, bidirectional=rnn.bidirectional, batch_first=True).double()
    ref.load_state_dict({k: v.detach().double().cpu() for k, v in rnn.state_dict().items()})
    x = x.detach().double().cpu().requires_grad_()
    D = 2 if rnn.bidirectional else 1
    out = torch.zeros(x.shape[0], D * rnn.hidden_size, dtype=torch.float64)
    live = [(b, s, n) for b, s, n in table.tolist() if n > 0]
    if live:
        rows = torch.tensor([[b + min(t, n - 1) * s for t in range(cap)] for b, s, n in live])
        packed = pack_padded_sequence(x[rows], torch.tensor([n for _, _, n in live]), batch_first=True, enforce_sorted=False)
        h, _ = pad_packed_sequence(ref(packed)[0], batch_first=True, total_length=cap)
        for j, (b, s, n) in enumerate(live):
            idx = torch.tensor([b + t * s for t in range(n)])
            out = out.index_put((idx,), h[j, :n])
    return ref, x, out


def _table(nseq, T, stride, counts):
    """``nseq`` sequences of room ``T``: stride 1: one after the other; stride > 1: interleaved in groups of ``stride`` (``nseq`` a multiple
    of it: every row belongs to a sequence, as the weight-gradient GEMMs behind the kernel require)."""
    assert stride == 1 or nseq % stride == 0
    rows = []
    for i in range(nseq):
        base = i * T if stride == 1 else (i // stride) * stride * T + i % stride
        rows.append([base, stride, counts[i % len(counts)]])
    total = nseq * T if stride == 1 else -(-nseq // stride) * stride * T
    return torch.tensor(rows, dtype=torch.int32), total


@pytest.mark.parametrize('nseq,T,stride,H,N,bi', [
    (1, 1, 1, 4, 4, True), (3, 2, 1, 5, 3, True), (4, 7, 1, 20, 6, True), (3, 7, 3, 20, 6, False), (5, 7, 1, 40, 8, False),
    (9, 7, 3, 128, 16, True), (5, 2, 1, 128, 64, False), (5, 4, 1, 160, 12, True), (3, 3, 3, 130, 6, False), (4, 2, 1, 512, 8, True),
    (2, 2, 1, 1100, 4, False)])
def test_chunk_lstm_against_torch(nseq, T, stride, H, N, bi):
    from padertorch_amd.ops import dprnn
    torch.manual_seed(nseq * 100 + H)
    counts = [T, 0, 1, T, T - 1 if T > 1 else 1]
    table, rows = _table(nseq, T, stride, counts)
    rnn = torch.nn.LSTM(N, H, bidirectional=bi, batch_first=True).cuda()
    x = torch.randn(rows, N).cuda().requires_grad_()
    r = torch.randn(rows, (2 if bi else 1) * H)
    h = dprnn.chunk_lstm(x, table.cuda(), T, rnn)
    covered = torch.zeros(rows, dtype=torch.bool)
    for b, s, n in table.tolist():
        covered[[b + t * s for t in range(T)]] = True
    grads = torch.autograd.grad((h * (r * covered[:, None]).cuda()).sum(), [x] + list(rnn.parameters()))
    ref, xr, want = _lstm_reference(rnn, x, table, T)
    want_grads = torch.autograd.grad((want * r.double()).sum(), [xr] + list(ref.parameters()))
    close('h', h[covered.cuda()], want[covered], VALUE)
    on_step = torch.zeros(rows, dtype=torch.bool)
    for b, s, n in table.tolist():
        on_step[[b + t * s for t in range(n)]] = True
    assert torch.all(h[(covered & ~on_step).cuda()] == 0)
    close('dx', grads[0][covered.cuda()], want_grads[0][covered], GRAD)
    for (n, _), g, w in zip(rnn.named_parameters(), grads[1:], want_grads[1:]):
        close('d ' + n, g, w, GRAD)


def test_chunk_lstm_state_is_isolated():
    """NaN in the gate rows of other sequences and of skipped steps reaches no valid output; skipped rows are exactly zero."""
    T, H, nseq = 5, 20, 6
    torch.manual_seed(5)
    table = torch.tensor([[i * T, 1, n] for i, n in enumerate([T, 0, 2, T, 1, 3])], dtype=torch.int32)
    rows = (nseq + 1) * T                                               # the last T rows belong to no sequence
    rnn = torch.nn.LSTM(H, H, bidirectional=True).cuda()
    gates = torch.randn(rows, 8 * H).cuda()
    args = (rnn.weight_hh_l0.detach(), rnn.weight_hh_l0_reverse.detach(), rnn.bias_hh_l0.detach(), rnn.bias_hh_l0_reverse.detach())
    h0, c0 = torch.ops.ptmi.chunk_lstm_forward(gates.clone(), *args, table.cuda(), T, H)
    on_step = torch.zeros(rows, dtype=torch.bool)
    for b, s, n in table.tolist():
        on_step[b:b + n] = True
    poisoned = gates.clone()
    poisoned[~on_step.cuda()] = float('nan')
    # one sequence alone: only its rows are clean
    alone = torch.full_like(gates, float('nan'))
    alone[0:T] = gates[0:T]
    h1, _ = torch.ops.ptmi.chunk_lstm_forward(poisoned, *args, table.cuda(), T, H)
    h2, _ = torch.ops.ptmi.chunk_lstm_forward(alone, *args, table[:1].cuda(), T, H)
    assert torch.equal(h1[on_step.cuda()], h0[on_step.cuda()]) and not torch.isnan(h0[:nseq * T]).any()
    assert torch.equal(h2[:T], h0[:T])
    skipped = ~on_step
    skipped[nseq * T:] = False
    assert torch.all(h1[skipped.cuda()] == 0)


@pytest.mark.parametrize('H', [20, 160])
def test_chunk_lstm_backward_is_isolated(H):
    """The backward kernel reads dh and the saved state on the rows of its sequences' steps only: NaN in dh, the gates, h and c of every
    other row changes nothing, and d gates / hprev are exactly zero on the skipped rows of the table."""
    T, nseq = 5, 6
    torch.manual_seed(6)
    counts = [T, 0, 2, T, 1, 3]
    table = torch.tensor([[i * T, 1, n] for i, n in enumerate(counts)], dtype=torch.int32).cuda()
    rows = (nseq + 1) * T                                               # the last T rows belong to no sequence
    rnn = torch.nn.LSTM(H, H, bidirectional=True).cuda()
    w = (rnn.weight_hh_l0.detach(), rnn.weight_hh_l0_reverse.detach())
    b = (rnn.bias_hh_l0.detach(), rnn.bias_hh_l0_reverse.detach())
    acts = torch.randn(rows, 8 * H).cuda()
    h, c = torch.ops.ptmi.chunk_lstm_forward(acts, w[0], w[1], b[0], b[1], table, T, H)
    dh = torch.randn(rows, 2 * H).cuda()
    on_step = torch.zeros(rows, dtype=torch.bool)
    for i, n in enumerate(counts):
        on_step[i * T:i * T + n] = True
    on, off = on_step.cuda(), (~on_step).cuda()
    clean = acts.clone()
    hprev0 = torch.ops.ptmi.chunk_lstm_backward(clean, dh, w[0], w[1], h, c, table, T, H)
    dirty, dh1, h1, c1 = acts.clone(), dh.clone(), h.clone(), c.clone()
    for t in (dirty, dh1, h1, c1):
        t[off] = float('nan')
    hprev1 = torch.ops.ptmi.chunk_lstm_backward(dirty, dh1, w[0], w[1], h1, c1, table, T, H)
    assert not torch.isnan(clean[on]).any() and float(clean[on].abs().max()) > 0
    assert torch.equal(dirty[on], clean[on]) and torch.equal(hprev1[on], hprev0[on])
    skipped = off.clone()
    skipped[nseq * T:] = False
    assert torch.all(dirty[skipped] == 0) and torch.all(hprev1[skipped] == 0)
    assert torch.isnan(dirty[nseq * T:]).all()                           # rows of no sequence are not touched


# ---------------------------------------------------------------------------------------------------- segment / overlap-add
def test_segment_and_overlap_add_doctest_answers():
    from padertorch_amd.modules import overlap_add, segment

    def seg(n, hop, win, length):
        s, l = segment((1. + torch.arange(n))[None, :, None].cuda(), hop, win, torch.tensor(length))
        return s[0, 0].tolist(), int(l)

    full = [[0, 1, 3, 5], [0, 2, 4, 0], [1, 3, 5, 0], [2, 4, 0, 0]]
    assert seg(5, 2, 4, 5) == (full, 4) and seg(5, 2, 4, 4) == (full, 3) and seg(5, 2, 4, 3) == (full, 3)
    assert seg(4, 2, 4, 4) == ([[0, 1, 3], [0, 2, 4], [1, 3, 0], [2, 4, 0]], 3)
    assert seg(3, 2, 4, 3) == ([[0, 1, 3], [0, 2, 0], [1, 3, 0], [2, 0, 0]], 3)
    five = torch.arange(5.)[None, :, None].cuda()
    for hop, shape, length in ((3, (1, 1, 4, 2), 2), (1, (1, 1, 4, 8), 8)):
        s, l = segment(five, hop, 4, torch.tensor(5))
        assert tuple(s.shape) == shape and int(l) == length
    s, l = segment(torch.ones(1, 7912, 64).cuda(), 50, 100, torch.tensor([7912]))
    assert tuple(s.shape) == (1, 64, 100, 160) and l.tolist() == [160]
    a = torch.arange(50.)[None, :, None].cuda()
    added = overlap_add(segment(a, 10, 20)[0], 10, unpad=True)
    assert tuple(added.shape) == (1, 50, 1) and added[0, :, 0].tolist() == list(range(0, 100, 2))
    assert overlap_add(segment(five, 2, 4)[0], 2)[0, :, 0].tolist() == [0, 2, 4, 6, 8, 0]
    assert overlap_add(segment(five, 3, 4)[0], 3)[0, :, 0].tolist() == [0, 1, 4, 3, 4]
    assert overlap_add(segment(five, 3, 4)[0], 3, unpad=False)[0, :, 0].tolist() == [0, 0, 1, 4, 3, 4, 0]
    with pytest.raises(NotImplementedError, match='no backward kernel'):
        overlap_add(segment(five.clone().requires_grad_(), 3, 4)[0], 3, unpad=False)


@pytest.mark.parametrize('L,K,P', [(13, 6, 1), (13, 6, 3), (13, 6, 5), (3, 8, 4), (70, 9, 4)])
def test_segment_is_the_adjoint_of_overlap_add(L, K, P):
    from padertorch_amd.ops import dprnn
    torch.manual_seed(L + K + P)
    x = torch.randn(2, L, 5).cuda().requires_grad_()
    seg = dprnn.segment_rows(x, K, P)
    S = dprnn.num_chunks(L, K, P)
    assert seg.shape == (2, S, K, 5)
    pad = torch.nn.functional.pad(x.detach().cpu(), [0, 0, K - P, K - P + (S - 1) * P + K])
    want = torch.stack([pad[:, s * P:s * P + K] for s in range(S)], 1)
    assert torch.equal(seg.detach().cpu(), want)
    y = torch.randn(2, S, K, 5).cuda().requires_grad_()
    out = dprnn.overlap_add_rows(y, P)
    assert out.shape == (2, S * P - (K - P), 5)
    # <segment(x), y> == <x, overlap_add(y)[:L]> in fp64
    lhs = float((seg.detach().double() * y.detach().double()).sum())
    rhs = float((x.detach().double() * out.detach().double()[:, :L]).sum())
    assert abs(lhs - rhs) <= 1e-5 * max(abs(lhs), 1.), (lhs, rhs)
    gx, = torch.autograd.grad((seg * y.detach()).sum(), x)
    close('d segment', gx, out.detach().double().cpu()[:, :L], VALUE)
    r = torch.randn_like(out)
    gy, = torch.autograd.grad((out * r).sum(), y)
    assert torch.equal(gy, dprnn.segment_rows(r, K, P))


# ---------------------------------------------------------------------------------------------------- norm + mask + residual
@pytest.mark.parametrize('N', [1, 63, 64, 65])
def test_norm_residual_against_fp64(N):
    B, S, K = 3, 4, 5
    torch.manual_seed(N)
    chunks = torch.tensor([4, 0, 2], dtype=torch.int32)                  # the second example is invalid throughout
    z = torch.randn(B * S * K, N)
    z[7] = 3.                                                           # a constant row: var = 0
    res, gy = torch.randn(B * S * K, N), torch.randn(B * S * K, N)
    gamma, beta = torch.rand(N) + 0.5, torch.rand(N) - 0.5
    valid = (torch.arange(S)[None, :, None] < chunks[:, None, None]).expand(B, S, K).reshape(-1, 1)
    zd, gd, bd = z.double().requires_grad_(), gamma.double().requires_grad_(), beta.double().requires_grad_()
    rd = res.double().requires_grad_()
    want = torch.nn.functional.layer_norm(zd, (N,), gd, bd, 1e-5) * valid + rd
    wants = torch.autograd.grad((want * gy.double()).sum(), [zd, rd, gd, bd])
    y, stats = torch.ops.ptmi.dprnn_norm_residual_forward(z.cuda(), res.cuda(), gamma.cuda(), beta.cuda(), chunks.cuda(), S, K, 1e-5)
    dz, dres, dparams = torch.ops.ptmi.dprnn_norm_residual_backward(gy.cuda(), z.cuda(), stats, gamma.cuda(), chunks.cuda(), S, K)
    close('y', y, want, VALUE)
    assert torch.equal(y.cpu()[~valid[:, 0]], res[~valid[:, 0]])
    if N == 1:          # a row of one element is its own mean: the gradient is exactly zero (torch's fp64 result is round-off, 1e-15)
        assert torch.all(dz == 0) and float(wants[0].abs().max()) < 1e-12
    else:
        close('dz', dz, wants[0], GRAD)
    assert torch.all(dz.cpu()[~valid[:, 0]] == 0)
    assert torch.equal(dres.cpu(), gy)
    if N == 1:          # ... and its normalised value is exactly zero, so is d gamma
        assert torch.all(dparams[:N] == 0) and float(wants[2].abs().max()) < 1e-12
    else:
        close('d gamma', dparams[:N], wants[2], GRAD)
    close('d beta', dparams[N:], wants[3], GRAD)
    again = torch.ops.ptmi.dprnn_norm_residual_backward(gy.cuda(), z.cuda(), stats, gamma.cuda(), chunks.cuda(), S, K)[2]
    assert torch.equal(again, dparams)
    free, _ = torch.ops.ptmi.dprnn_norm_residual_forward(z.cuda(), res.cuda(), gamma.cuda(), beta.cuda(), None, S, K, 1e-5)
    close('y without lengths', free, torch.nn.functional.layer_norm(z.double(), (N,), gamma.double(), beta.double(), 1e-5) + res.double(), VALUE)


SLAB_ROWS = 128             # kDpSlabRows of csrc/dprnn.hip: rows per partial of the column sums


@pytest.mark.parametrize('C', [5, 70])
def test_colsum_over_many_slabs_against_fp64(C):
    """5 1/4 slabs of rows and a width that is no multiple of 64: every one of the four chains of colreduce_kernel (csrc/reduce.h) adds
    more than one partial, the last slab and the last column block are ragged.  Both store forms: one output (the fc bias) and the pair
    (b_ih and b_hh), from a contiguous tensor and from columns of a wider one.  The sums are fp64 inside and rounded once: VALUE."""
    rows = 5 * SLAB_ROWS + SLAB_ROWS // 4 + 5
    torch.manual_seed(C)
    wide = torch.randn(rows, C + 3).cuda()
    for name, x in (('contiguous', wide[:, :C].contiguous()), ('strided', wide[:, 2:2 + C])):
        one = torch.ops.ptmi.dprnn_colsum(x)
        a, b = torch.ops.ptmi.dprnn_colsum_pair(x)
        close(f'colsum {name} C={C}', one, x.cpu().double().sum(0), VALUE)
        assert a.data_ptr() != b.data_ptr() and torch.equal(a, one) and torch.equal(b, one)


# ---------------------------------------------------------------------------------------------------- full width
def _block_fp64(block, x, S_b, K, P):
    """One DPRNN block on ``x [B, S, K, N]`` in fp64 on the CPU from torch.nn.LSTM / Linear / LayerNorm with the block's parameters;
    returns the output and the fp64 parameters in the order of ``block.named_parameters()``."""
    from torch.nn.utils.rnn import pack_padded_sequence, pad_packed_sequence
    B, S, _, N = x.shape
    valid = (torch.arange(S)[None, :] < torch.tensor(S_b)[:, None])
    leaves = []
    for path, chunk in (('intra', block.intra_chunk_rnn), ('inter', block.inter_chunk_rnn)):
        rnn = torch.nn.LSTM(N, chunk.rnn.hidden_size, bidirectional=chunk.rnn.bidirectional, batch_first=True).double()
        rnn.load_state_dict({k: v.detach().double().cpu() for k, v in chunk.rnn.state_dict().items()})
        w, b = chunk.fc.weight.detach().double().cpu().requires_grad_(), chunk.fc.bias.detach().double().cpu().requires_grad_()
        g, be = chunk.norm.weight.detach().double().cpu().requires_grad_(), chunk.norm.bias.detach().double().cpu().requires_grad_()
        leaves += [p for _, p in rnn.named_parameters()] + [w, b, g, be]
        assert [n for n, _ in chunk.named_parameters()] == ['rnn.' + n for n, _ in rnn.named_parameters()] + [
            'fc.weight', 'fc.bias', 'norm.weight', 'norm.bias']
        if path == 'intra':
            h = rnn(x.reshape(B * S, K, N))[0].reshape(B, S, K, -1)
        else:
            seqs = x.permute(0, 2, 1, 3).reshape(B * K, S, N)
            lens = torch.tensor(S_b).repeat_interleave(K)
            h, _ = pad_packed_sequence(rnn(pack_padded_sequence(seqs, lens, batch_first=True, enforce_sorted=False))[0],
                                       batch_first=True, total_length=S)
            h = h.reshape(B, K, S, -1).permute(0, 2, 1, 3)
        z = torch.nn.functional.layer_norm(h @ w.t() + b, (N,), g, be, chunk.norm.eps)
        x = z * valid[:, :, None, None] + x
    return x, leaves


def test_full_width_block_against_fp64():
    """H = 128, K = 100: the register-resident kernels at their full size, 100-step intra and 6-step inter sequences, through the fused
    block backward.  Lengths [230, 170, 170]: one full example and two EQUAL shorter ones whose last chunk is masked (the case the
    reference itself cannot run when no example is full, make_golden_dprnn.py)."""
    from padertorch_amd.modules import DPRNN
    from padertorch_amd.ops import dprnn
    torch.manual_seed(11)
    N, H, K, P, B, L, lengths = 64, 128, 100, 50, 3, 230, [230, 170, 170]
    net = DPRNN(N, H, K, P, num_blocks=1).cuda()
    with torch.no_grad():
        for n, p in net.named_parameters():
            if '.norm.' in n:
                p.copy_(torch.rand_like(p) + (0.5 if n.endswith('weight') else -0.5))
    x = torch.randn(B, L, N).cuda().requires_grad_()
    r = torch.randn(B, dprnn.num_chunks(L, K, P) * P - (K - P), N)
    y = net(x, lengths)
    grads = torch.autograd.grad((y * r.cuda()).sum(), [x] + list(net.parameters()))
    S = dprnn.num_chunks(L, K, P)
    S_b = dprnn.chunk_counts(lengths, K, P).tolist()
    assert S_b == [6, 5, 5] and S == 6
    xd = x.detach().double().cpu().requires_grad_()
    pad = torch.nn.functional.pad(xd, [0, 0, K - P, K - P + (S - 1) * P + K])
    seg = torch.stack([pad[:, s * P:s * P + K] for s in range(S)], 1)
    out, leaves = _block_fp64(net.dprnn_blocks[0], seg, S_b, K, P)
    full = torch.zeros(B, (S - 1) * P + K, N, dtype=torch.float64)
    for s in range(S):
        full[:, s * P:s * P + K] = full[:, s * P:s * P + K] + out[:, s]
    want = full[:, K - P:-(K - P)]
    close('full width y', y, want.detach(), VALUE)
    wants = torch.autograd.grad((want * r.double()).sum(), [xd] + leaves)
    close('full width dx', grads[0], wants[0], GRAD)
    for (n, _), g, w in zip(net.named_parameters(), grads[1:], wants[1:]):
        close('full width d ' + n, g, w, GRAD)


# ---------------------------------------------------------------------------------------------------- the models around it
def _default_tasnet():
    from padertorch_amd.contrib.examples.source_separation.tasnet import TasDecoder, TasEncoder, TasNet
    from padertorch_amd.modules import DPRNN
    torch.manual_seed(3)
    return TasNet(TasEncoder(16, 64), DPRNN(64, 128, 100, 50, 6), TasDecoder(16, 64))


def test_default_tasnet_trains_a_step_through_the_trainer(tmp_path):
    import padertorch_amd as pt
    model = _default_tasnet()
    t = pt.Trainer(model, tmp_path, pt.optimizer.Adam(gradient_clipping=1.), loss_weights={'si-sdr': 1., 'log-mse': 0., 'log1p-mse': 0.})
    t.to('cuda')
    rng = np.random.RandomState(0)
    s = torch.from_numpy(rng.randn(2, 2, 4000).astype(np.float32)).cuda()
    batch = dict(y=s.sum(1), s=s, num_samples=[4000, 3000])
    before = {k: v.clone() for k, v in model.state_dict().items()}
    losses = []
    for _ in range(2):
        loss, _, _, _ = t.train_step(t.model, batch, 'cuda')
        loss.backward()
        t.optimizer_step()
        losses.append(float(loss))
    torch.cuda.synchronize()
    assert all(np.isfinite(losses)), losses
    after = model.state_dict()
    moved = [k for k in before if not torch.equal(before[k], after[k])]
    assert len(moved) == len(before), sorted(set(before) - set(moved))       # every parameter received a gradient and a step
    assert all(torch.isfinite(v).all() for v in after.values())


def test_one_and_rest_pit_on_dprnn():
    from padertorch_amd.contrib.examples.source_separation.or_pit import OneAndRestPIT
    from padertorch_amd.contrib.examples.source_separation.tasnet import TasDecoder, TasEncoder, TasNet
    from padertorch_amd.modules import DPRNN
    torch.manual_seed(4)
    separator = TasNet(TasEncoder(16, 12), DPRNN(12, 20, 10, 5, 1), TasDecoder(16, 12), num_speakers=2, additional_out_size=4)
    net = OneAndRestPIT(separator, flag_units=4).cuda()
    rng = np.random.RandomState(1)
    s = torch.from_numpy(rng.randn(2, 3, 800).astype(np.float32)).cuda()
    batch = dict(y=s.sum(1), s=s, num_samples=[800, 800], num_speakers=[3, 3])
    out = net(batch)
    review = net.review(batch, out)
    assert torch.isfinite(review['loss'])
    grads = torch.autograd.grad(review['loss'], list(net.parameters()), allow_unused=True)
    got = [g for g in grads if g is not None]
    assert got and all(torch.isfinite(g).all() for g in got)
    dprnn_grads = [g for (n, _), g in zip(net.named_parameters(), grads) if 'dprnn_blocks' in n]
    assert dprnn_grads and all(g is not None and float(g.abs().max()) > 0 for g in dprnn_grads)
