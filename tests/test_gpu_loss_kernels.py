"""The PIT, deep-clustering and time-domain loss kernels (``csrc/pit_loss.hip``, ``csrc/dc_loss.hip``, ``csrc/td_loss.hip``) path by
path against fp64 references on the CPU (GPU, through the public wrappers and ``torch.ops.ptmi.*``).

Every case names the branch it runs by its shape and arguments:

* PIT: ``pit_pairwise_kernel<1>`` (K = 1); ``pit_pairwise_generic_kernel`` + ``pit_assign_kernel`` at K = 6, 7, 8 (``kMaxK``); the
  status error at K = 9; ``nvar == 1`` with an observation and lengths; time-major data; strided views; the ``sse`` output; poisoned
  padding in forward and backward.
* Deep clustering: K > ``kDcKX`` and D = 32 on the generic kernels, the three ``EX`` instantiations at their edges, lengths on the
  256-row tile and 2048-row chunk edges, both non-default layouts with lengths, channel and time views (``x_span`` from strides),
  poisoned padding on the buffer-load, generic register and generic LDS (host zero-fill) backward forms.
* Time domain: the five sums themselves, ``td_stats_row_kernel`` with lengths, ``td_lincomb_kernel<1..8>`` on its ``float4`` and
  scalar paths, lengths on the 1024-sample chunk edge / not a multiple of 4 / above T, views, poisoned tails, one end-to-end case.

Exact permutation comparisons are preceded by an assertion, on the reference's fp64 values, that the best and the second-best
candidate differ by at least ``GAP`` relative (more than 100 fp32 ulps): no correctly rounded fp32 comparison can then pick another
permutation.  Poison and view cases assert bitwise equality with the clean / contiguous run."""
import functools
import itertools

import numpy as np
import pytest
import torch

from oracle import losses_np
from test_gpu_td import close_grad

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
GAP = 1e-5
POISONS = [float('nan'), 1e30]


def dev(a):
    return torch.tensor(a).to(DEV)                    # a copy: the shared cases are read-only


def cpu64(a):
    return torch.tensor(a, dtype=torch.float64)


def lens_dev(lens):
    return torch.tensor(lens, dtype=torch.int32, device=DEV)


@functools.lru_cache(maxsize=None)
def perm_table(K):
    return np.array(list(itertools.permutations(range(K))), dtype=np.int64)


def walk_permutations(L):
    """``L [K, K]``: loss of estimate i against target j.  Candidates in ``itertools.permutations`` order (estimate ``p[j]`` with
    target ``j``, mean over j), first minimum wins.  Returns (best value, permutation, relative gap to the second-best candidate)."""
    K = L.shape[0]
    perms = perm_table(K)
    cands = L[perms, np.arange(K)].mean(1)
    best = int(np.argmin(cands))
    gap = np.inf
    if len(cands) > 1:
        second = np.partition(cands, 1)[1]
        gap = (second - cands[best]) / abs(cands[best])
    return cands[best], [int(p) for p in perms[best]], gap


# ======================================================================================================================== PIT
PIT_LENS = (17, 16, 9, 8, 1)          # T = 17: three 8-frame chunks (kTChunk), the last one holds a single frame
# RandomState(K) like test_fused_review_vs_oracle, except where that draw has two candidates closer than GAP in fp64 (K = 6, F = 33,
# PIT_LENS: 1.3e-6 relative): the seed is chosen on the reference's values, the exact permutation comparison is never relaxed
PIT_SEEDS = {(6, 33): 106}


@functools.lru_cache(maxsize=None)
def pit_case(K, F, lens=PIT_LENS):
    """The recipe of ``test_gpu_pit.test_fused_review_vs_oracle`` and its fp64 reference: per variant (0: MSE, 1: ideal phase
    sensitive) the per-example loss, the permutation (walked over the pairwise matrix of the oracle) and the candidate gap."""
    rng = np.random.RandomState(PIT_SEEDS.get((K, F), K))
    B, T = len(lens), max(lens)
    mask = np.abs(rng.standard_normal((B, T, K, F))).astype(np.float32)
    Y = np.abs(rng.standard_normal((B, T, F))).astype(np.float32)
    X = np.abs(rng.standard_normal((B, T, K, F))).astype(np.float32)
    C = np.cos(rng.uniform(-3, 3, (B, T, K, F))).astype(np.float32)
    ex = np.zeros((B, 2))
    perms = [[None, None] for _ in lens]
    gap = np.inf
    for b, l in enumerate(lens):
        est = mask[b, :l].astype(np.float64) * Y[b, :l].astype(np.float64)[:, None, :]
        tgt = X[b, :l].astype(np.float64)
        for v, g in enumerate((tgt, tgt * C[b, :l].astype(np.float64))):
            ex[b, v], perms[b][v], gp = walk_permutations(losses_np.pairwise_losses(est, g, axis=-2))
            gap = min(gap, gp)
    for a in (mask, Y, X, C, ex):
        a.setflags(write=False)
    return dict(mask=mask, Y=Y, X=X, C=C, lens=lens, ex=ex, perms=perms, gap=gap)


def pit_ref_grad(case, weights):
    """fp64 autograd gradient w.r.t. the mask of ``sum_v weights[v] * batch mean of the variant's loss`` at the reference permutations."""
    lens = case['lens']
    B = len(lens)
    mt = cpu64(case['mask']).requires_grad_(True)
    tot = 0
    for b, l in enumerate(lens):
        est = mt[b, :l] * cpu64(case['Y'][b, :l])[:, None, :]
        tg = cpu64(case['X'][b, :l])
        for v, w in enumerate(weights):
            g = tg if v == 0 else tg * cpu64(case['C'][b, :l])
            tot = tot + w * ((est[:, case['perms'][b][v]] - g) ** 2).mean() / B
    tot.backward()
    return mt.grad.numpy()


def pit_run(mask, Y, X, C, ld, weights=(0.25, 1.0), **kw):
    """One forward + backward of ``pit_mse_ips_losses``; ``mask`` is the differentiable leaf (or a view of it)."""
    from padertorch_amd.ops.losses import pit_mse_ips_losses
    loss, perm, ex = pit_mse_ips_losses(mask, Y, X, C, ld, **kw)
    sum(w * loss[v] for v, w in enumerate(weights[:loss.shape[0]])).backward()
    return loss.detach(), perm, ex


@pytest.mark.parametrize('F', [7, 33])
@pytest.mark.parametrize('K', [1, 6, 7, 8])
def test_pit_one_and_many_sources_vs_oracle(K, F):
    """K = 1 is ``pit_pairwise_kernel<1>``; K = 6, 7, 8 are ``pit_pairwise_generic_kernel`` and up to 8! = 40320 permutations in one
    thread of ``pit_assign_kernel``.  Loss, per-example loss, both permutations (exact) and the gradient, both mask layouts; the
    tolerances of ``test_fused_review_vs_oracle``."""
    case = pit_case(K, F)
    lens = case['lens']
    assert case['gap'] >= GAP, case['gap']                 # precondition of the exact permutation comparison below
    want_grad = pit_ref_grad(case, (0.25, 1.0))
    ld = lens_dev(lens)
    for batch_first in (True, False):
        m = dev(case['mask']) if batch_first else dev(case['mask']).transpose(0, 1).contiguous()
        m.requires_grad_(True)
        loss, perm, ex = pit_run(m, dev(case['Y']), dev(case['X']), dev(case['C']), ld, mask_batch_first=batch_first)
        np.testing.assert_allclose(loss.cpu().numpy(), case['ex'].mean(0), rtol=2e-6)
        np.testing.assert_allclose(ex.cpu().numpy(), case['ex'], rtol=2e-6)
        assert perm.tolist() == case['perms']
        got = m.grad if batch_first else m.grad.transpose(0, 1)
        np.testing.assert_allclose(got.cpu().numpy(), want_grad, atol=1e-7, rtol=1e-4)


def test_pit_nine_sources_is_a_status_error():
    """K = 9 > ``kMaxK``: ``ptmi_pit_assign`` returns ``PTMI_E_UNSUPPORTED`` (after the pairwise launch) and the wrapper raises the
    library's status error instead of returning a loss."""
    from padertorch_amd.ops.losses import pit_mse_ips_losses
    g = torch.Generator().manual_seed(9)
    B, T, K, F = 2, 9, 9, 7
    mask, X, C = (torch.rand(B, T, K, F, generator=g).to(DEV) for _ in range(3))
    Y = torch.rand(B, T, F, generator=g).to(DEV)
    with pytest.raises(RuntimeError, match='ptmi_pit_assign'):
        pit_mse_ips_losses(mask, Y, X, C, lens_dev([9, 4]))
    torch.cuda.synchronize()


def test_pit_mse_variant_alone_with_lengths():
    """``cos_phase_difference=None`` with an observation and ragged lengths (``nvar == 1``): one loss, ``perm [B, 1, K]``, value and
    gradient against the oracle's MSE variant alone."""
    case = pit_case(3, 33)
    lens = case['lens']
    B, K = len(lens), 3
    assert case['gap'] >= GAP, case['gap']
    m = dev(case['mask']).requires_grad_(True)
    loss, perm, ex = pit_run(m, dev(case['Y']), dev(case['X']), None, lens_dev(lens), weights=(1.0,))
    assert list(loss.shape) == [1] and list(perm.shape) == [B, 1, K] and list(ex.shape) == [B, 1]
    np.testing.assert_allclose(loss.item(), case['ex'][:, 0].mean(), rtol=2e-6)
    np.testing.assert_allclose(ex[:, 0].cpu().numpy(), case['ex'][:, 0], rtol=2e-6)
    assert perm[:, 0].tolist() == [p[0] for p in case['perms']]
    np.testing.assert_allclose(m.grad.cpu().numpy(), pit_ref_grad(case, (1.0,)), atol=1e-7, rtol=1e-4)


@pytest.mark.parametrize('K', [2, 5])
def test_pit_time_major_data_is_bitwise_the_batch_major_call(K):
    """``data_batch_first=False``: observation ``[T, B, F]``, target and phase ``[T, B, K, F]``, with both mask layouts.  The reduction
    order does not depend on the layout, so everything is bitwise the batch-major call on the same data."""
    case = pit_case(K, 33)
    ld = lens_dev(case['lens'])
    Y, X, C = dev(case['Y']), dev(case['X']), dev(case['C'])
    Yt, Xt, Ct = (a.transpose(0, 1).contiguous() for a in (Y, X, C))
    for batch_first in (True, False):
        m0 = dev(case['mask']) if batch_first else dev(case['mask']).transpose(0, 1).contiguous()
        m1 = m0.clone()
        m0.requires_grad_(True)
        m1.requires_grad_(True)
        want = pit_run(m0, Y, X, C, ld, mask_batch_first=batch_first)
        got = pit_run(m1, Yt, Xt, Ct, ld, mask_batch_first=batch_first, data_batch_first=False)
        for a, b in zip(got, want):
            assert torch.equal(a, b)
        assert torch.equal(m1.grad, m0.grad)
    np.testing.assert_allclose(want[0].cpu().numpy(), case['ex'].mean(0), rtol=2e-6)     # ... and it is the right answer


@pytest.mark.parametrize('K', [3, 5])
def test_pit_views_of_a_larger_buffer(K):
    """Mask, observation, target and phase are each ``big[:, 1:1 + T]`` of a buffer with T + 3 frames (batch and time strides are not
    the packed ones); the frames outside the view are NaN.  Loss, permutation, per-example loss and the gradient read through the same
    view are bitwise the contiguous call."""
    case = pit_case(K, 33)
    T = max(case['lens'])
    ld = lens_dev(case['lens'])

    def framed(a):
        big = torch.full((a.shape[0], T + 3) + tuple(a.shape[2:]), float('nan'), device=DEV)
        big[:, 1:1 + T] = dev(a)
        return big
    m0 = dev(case['mask']).requires_grad_(True)
    want = pit_run(m0, dev(case['Y']), dev(case['X']), dev(case['C']), ld)
    big_m = framed(case['mask']).requires_grad_(True)
    views = [framed(case[k])[:, 1:1 + T] for k in ('Y', 'X', 'C')]
    assert not any(v.is_contiguous() for v in views)
    got = pit_run(big_m[:, 1:1 + T], *views, ld)
    for a, b in zip(got, want):
        assert torch.equal(a, b)
    assert torch.equal(big_m.grad[:, 1:1 + T], m0.grad)
    assert not big_m.grad[:, :1].any() and not big_m.grad[:, 1 + T:].any()


@pytest.mark.parametrize('F', [1, 257])
@pytest.mark.parametrize('K', [2, 4, 5, 8])
def test_pit_sse_vs_fp64_pairwise_sums(K, F):
    """The ``sse [B, nvar, K, K]`` output of ``torch.ops.ptmi.pit_loss_forward`` (K = 2, 4: template kernel; 5, 8: generic kernel)
    against the pairwise sums in fp64, with ``e = mask * Y`` and ``d = e - g`` exact in fp64.

    Bound per entry: ``2 * (2^-23 * sum |d| (|e| + |d|) + (ceil(8 F / 256) + 2) * 2^-24 * sum d^2)``.  Derivation: the kernel rounds
    ``e`` once (2^-24 |e|) and ``d`` once (2^-24 |d|), whether or not the compiler contracts them, so ``d^2`` is off by at most
    ``2 |d| * 2^-24 (|e| + |d|)``; the square is rounded once (2^-24 d^2); a thread then adds at most ``ceil(8 F / 256)`` terms of its
    8-frame chunk in fp32 (2^-24 of the running sum each) before the sums go to fp64; the whole is doubled.  The 64-lane butterfly that
    follows the per-thread sums is fp32 too (at most 6 more additions): the doubling covers it at F = 257 (2 * 11 >= 9 + 6 + 1), and at
    F = 1 a chunk has at most 8 terms, one per thread, so the per-thread sum is exact and at most 3 butterfly additions are inexact
    (2 * 3 >= 3 + 1).  The phase-sensitive variant compares with ``h = g * cos``, which the kernel rounds to fp32 or contracts into the
    subtraction: at most 2^-24 |h| more on ``d``, i.e. ``2^-23 |d| |h|`` more in the first sum of that variant only."""
    lens = (17, 9, 8, 1)
    case = pit_case(K, F, lens)
    B, T = len(lens), max(lens)
    m, Y, X, C = dev(case['mask']), dev(case['Y']), dev(case['X']), dev(case['C'])
    strides = [m.stride(0), m.stride(1), Y.stride(0), Y.stride(1), X.stride(0), X.stride(1)]
    _, _, _, sse = torch.ops.ptmi.pit_loss_forward(m, Y, X, C, lens_dev(lens), B, T, K, F, strides)
    assert list(sse.shape) == [B, 2, K, K] and sse.dtype == torch.float64
    sse = sse.cpu().numpy()
    adds = -(-8 * F // 256)
    for b, l in enumerate(lens):
        e = (case['mask'][b, :l].astype(np.float64) * case['Y'][b, :l].astype(np.float64)[:, None, :])[:, :, None, :]   # [l, i, 1, F]
        tgt = case['X'][b, :l].astype(np.float64)
        for v, g in enumerate((tgt, tgt * case['C'][b, :l].astype(np.float64))):
            g = g[:, None, :, :]                                                                                       # [l, 1, j, F]
            d = e - g
            h = np.abs(g) if v == 1 else 0.
            want = (d * d).sum((0, 3))
            bound = 2 * (2. ** -23 * (np.abs(d) * (np.abs(e) + np.abs(d) + h)).sum((0, 3)) + (adds + 2) * 2. ** -24 * want)
            err = np.abs(sse[b, v] - want)
            assert (err <= bound).all(), (b, v, float((err / bound).max()))


@pytest.mark.parametrize('F', [7, 33])
@pytest.mark.parametrize('K', [2, 5])
def test_pit_poisoned_padding(K, F):
    """Every frame at or beyond its example's length holds NaN, then 1e30, in mask, observation, target and phase; both mask layouts.
    Forward and backward are guarded by ``t < T_b``: everything is bitwise the clean run and the gradient in the padding is zero."""
    case = pit_case(K, F)
    lens = case['lens']
    ld = lens_dev(lens)

    def run(poison, batch_first):
        ts = [dev(case[k]) for k in ('mask', 'Y', 'X', 'C')]
        if poison is not None:
            for t in ts:
                for b, l in enumerate(lens):
                    t[b, l:] = poison
        m = (ts[0] if batch_first else ts[0].transpose(0, 1).contiguous()).requires_grad_(True)
        out = pit_run(m, *ts[1:], ld, mask_batch_first=batch_first)
        return out, (m.grad if batch_first else m.grad.transpose(0, 1))
    for batch_first in (True, False):
        clean, clean_grad = run(None, batch_first)
        for poison in POISONS:
            out, grad = run(poison, batch_first)
            for a, b in zip(out, clean):
                assert torch.equal(a, b)
            for b, l in enumerate(lens):
                assert torch.equal(grad[b, :l], clean_grad[b, :l])
                assert not grad[b, l:].any() and not torch.isnan(grad[b, l:]).any()


# ============================================================================================================ deep clustering
@functools.lru_cache(maxsize=None)
def dc_case(E, K, F, lens):
    """Embedding ``[T, B, E, F]``, one-hot target mask ``[B, T, K, F]`` and the fp64 reference of
    ``test_gpu_model.test_dc_loss_batched_shapes_vs_oracle``: per-example losses (oracle) and the gradient of their batch mean."""
    rng = np.random.RandomState(E * 100 + K)
    B, T = len(lens), max(lens)
    emb = rng.standard_normal((T, B, E, F)).astype(np.float32)
    tm = np.eye(K, dtype=np.float32)[rng.randint(0, K, (B, T, F))].transpose(0, 1, 3, 2).copy()
    ref = np.array([losses_np.deep_clustering_loss(emb[:l, b].transpose(0, 2, 1).reshape(-1, E),
                                                   tm[b, :l].transpose(0, 2, 1).reshape(-1, K)) for b, l in enumerate(lens)])
    xt = cpu64(emb).requires_grad_(True)
    tot = 0
    for b, l in enumerate(lens):
        X = xt[:l, b].permute(0, 2, 1).reshape(-1, E)
        Tm = cpu64(tm[b, :l]).permute(0, 2, 1).reshape(-1, K)
        N = X.shape[0]
        tot = tot + (((X.t() @ X) ** 2).sum() - 2 * ((X.t() @ Tm) ** 2).sum() + ((Tm.t() @ Tm) ** 2).sum()) / N ** 2 / B
    tot.backward()
    grad = xt.grad.numpy()
    for a in (emb, tm, ref, grad):
        a.setflags(write=False)
    return dict(emb=emb, tm=tm, lens=lens, ref=ref, grad=grad)


def dc_assert_vs_reference(case, ex, loss, grad):
    """The gates of ``test_dc_loss_batched_shapes_vs_oracle``; ``grad`` in the ``[T, B, E, F]`` layout."""
    np.testing.assert_allclose(ex.cpu().numpy(), case['ref'], rtol=3e-5)
    np.testing.assert_allclose(loss.item(), case['ref'].mean(), rtol=3e-5)
    g = grad.cpu().numpy()
    np.testing.assert_allclose(g, case['grad'], atol=1e-7 * max(1.0, float(np.abs(case['grad']).max())), rtol=3e-4)
    for b, l in enumerate(case['lens']):
        assert not g[l:, b].any()                      # padded frames get exactly zero


def dc_run(x, t, ld, **kw):
    """One forward + backward of ``dc_loss_batched``; ``x`` is the differentiable leaf (or a view of it)."""
    from padertorch_amd.ops.losses import dc_loss_batched
    loss, ex = dc_loss_batched(x, t, ld, **kw)
    loss.backward()
    return loss.detach(), ex


@pytest.mark.parametrize('E,K,F,lens', [
    (20, 9, 37, (9, 7, 2)),                # K > kDcKX = 8 with E <= 24: generic kernels, register backward
    (28, 4, 37, (9, 7, 2)),                # generic at the D = E + K = 32 limit
    (23, 9, 37, (9, 7, 2)),                # D = 32 through K
    (8, 8, 37, (9, 7, 2)),                 # EX = 8 full, K = kDcKX
    (16, 1, 37, (9, 7, 2)),                # EX = 16 full, K = 1
    (17, 2, 37, (9, 7, 2)),                # one past 16: EX = 24
    (4, 2, 64, (33, 32, 5, 4, 3)),         # rows 2112, 2048, 320, 256, 192: a full chunk, one tile into the second, exactly one tile
    (4, 2, 1, (2049, 2048, 257, 1)),       # the same edges one row at a time
])
def test_dc_kernel_families_and_tile_edges_vs_oracle(E, K, F, lens):
    """Ragged ``dc_loss_batched`` on the default layout: per-example value, batch mean and gradient against the fp64 oracle, padded
    frames exactly zero.  Rows 333, 259 and 74 of the family cases end inside the second, just past the first and inside the first
    256-row tile (``kDcTile``)."""
    case = dc_case(E, K, F, lens)
    x = dev(case['emb']).requires_grad_(True)
    loss, ex = dc_run(x, dev(case['tm']), lens_dev(lens))
    dc_assert_vs_reference(case, ex, loss, x.grad)


@pytest.mark.parametrize('E,K', [(20, 3), (25, 3)])
def test_dc_layouts_with_lengths(E, K):
    """``target_batch_first=False`` and ``embedding_batch_first=True`` with ragged lengths (fast and generic kernels): per-example
    losses bitwise the default-layout call on the same data, gradients equal after transposition."""
    case = dc_case(E, K, 37, (9, 7, 2))
    ld = lens_dev(case['lens'])
    x0 = dev(case['emb']).requires_grad_(True)
    t0 = dev(case['tm'])
    loss0, ex0 = dc_run(x0, t0, ld)
    dc_assert_vs_reference(case, ex0, loss0, x0.grad)
    for emb_bf, tgt_bf in ((False, False), (True, True), (True, False)):
        x = (dev(case['emb']).transpose(0, 1).contiguous() if emb_bf else dev(case['emb'])).requires_grad_(True)
        t = t0 if tgt_bf else t0.transpose(0, 1).contiguous()
        loss, ex = dc_run(x, t, ld, embedding_batch_first=emb_bf, target_batch_first=tgt_bf)
        assert torch.equal(ex, ex0) and torch.equal(loss, loss0)
        assert torch.equal(x.grad.transpose(0, 1) if emb_bf else x.grad, x0.grad)


@pytest.mark.parametrize('E', [20, 25])
def test_dc_embedding_views(E):
    """The embedding as channels ``2:2 + E`` of a ``[T, B, E + 5, F]`` tensor (``xs[1] != E * F``: ``x_span`` comes from the strides)
    and as frames ``1:1 + T`` of a longer batch-major tensor; everything outside the view is NaN.  E = 20: fast kernels, E = 25:
    generic.  Values bitwise the contiguous call, the gradient equal through the view and zero outside it."""
    K, F = 3, 37
    case = dc_case(E, K, F, (9, 7, 2))
    T, B = case['emb'].shape[:2]
    ld = lens_dev(case['lens'])
    t = dev(case['tm'])
    x0 = dev(case['emb']).requires_grad_(True)
    loss0, ex0 = dc_run(x0, t, ld)
    dc_assert_vs_reference(case, ex0, loss0, x0.grad)

    wide = torch.full((T, B, E + 5, F), float('nan'), device=DEV)
    wide[:, :, 2:2 + E] = dev(case['emb'])
    wide.requires_grad_(True)
    loss, ex = dc_run(wide[:, :, 2:2 + E], t, ld)
    assert torch.equal(ex, ex0) and torch.equal(loss, loss0)
    assert torch.equal(wide.grad[:, :, 2:2 + E], x0.grad)
    assert not wide.grad[:, :, :2].any() and not wide.grad[:, :, 2 + E:].any()

    x1 = dev(case['emb']).transpose(0, 1).contiguous().requires_grad_(True)
    loss1, ex1 = dc_run(x1, t, ld, embedding_batch_first=True)
    long = torch.full((B, T + 2, E, F), float('nan'), device=DEV)
    long[:, 1:1 + T] = x1.detach()
    long.requires_grad_(True)
    loss, ex = dc_run(long[:, 1:1 + T], t, ld, embedding_batch_first=True)
    assert torch.equal(ex, ex1) and torch.equal(loss, loss1) and torch.equal(ex, ex0)
    assert torch.equal(long.grad[:, 1:1 + T], x1.grad)
    assert not long.grad[:, :1].any() and not long.grad[:, 1 + T:].any()


@pytest.mark.parametrize('form', ['fast', 'generic-register', 'generic-lds'])
def test_dc_poisoned_padding(form):
    """NaN, then 1e30, in the padded frames of both embedding and target mask, on the three backward forms: (20, 3) buffer loads,
    (25, 3) generic register form, and a column-contiguous layout (embedding stored ``[T, B, F, E]``, mask ``[B, T, F, K]``) through
    ``torch.ops.ptmi.dc_loss_forward / _backward`` - no public wrapper reaches the LDS form with lengths - with the host zero-fill that
    ``_DcFn`` asks for there.  ``ex_loss``, ``loss`` and the gradient inside the lengths are bitwise the clean run, the gradient in
    the padding is exactly zero; the clean run itself is held to the fp64 reference."""
    E, K, F = (25, 3, 37) if form == 'generic-register' else (20, 3, 37)
    case = dc_case(E, K, F, (9, 7, 2))
    lens = case['lens']
    T, B = case['emb'].shape[:2]
    ld = lens_dev(lens)

    def run(poison):
        x, t = dev(case['emb']), dev(case['tm'])
        if poison is not None:
            for b, l in enumerate(lens):
                x[l:, b] = poison
                t[b, l:] = poison
        if form != 'generic-lds':
            x.requires_grad_(True)
            loss, ex = dc_run(x, t, ld)
            return loss, ex, x.grad
        xs, ts = x.permute(0, 1, 3, 2).contiguous(), t.permute(0, 1, 3, 2).contiguous()       # [T, B, F, E], [B, T, F, K]
        strides = [F * E, B * F * E, 1, E, T * F * K, F * K, 1, K]                              # (b, t, channel, f) of each
        loss, ex, gram = torch.ops.ptmi.dc_loss_forward(xs, ts, ld, B, T, E, K, F, strides)
        dx = torch.ops.ptmi.dc_loss_backward(xs, ts, gram, torch.ones(1, device=DEV), ld, B, T, E, K, F, strides, True)
        return loss[0], ex, dx.permute(0, 1, 3, 2)
    loss0, ex0, grad0 = run(None)
    dc_assert_vs_reference(case, ex0, loss0, grad0)
    for poison in POISONS:
        loss, ex, grad = run(poison)
        assert torch.equal(ex, ex0) and torch.equal(loss, loss0)
        for b, l in enumerate(lens):
            assert torch.equal(grad[:l, b], grad0[:l, b])
            assert not grad[l:, b].any() and not torch.isnan(grad[l:, b]).any()


# ================================================================================================================ time domain
TD_B = 7
TD_LENS = {
    2052: (2052, 1025, 1024, 1023, 5, 1, 2059),   # rows 16-byte aligned: float4 path, three 1024-sample chunks; 2059 > T is clamped
    1027: (1027, 1025, 1024, 1023, 5, 1, 1040),   # rows not 16-byte aligned: scalar path
    3: (3, 2, 1, 3, 1, 2, 9),                     # T < 4
}


@functools.lru_cache(maxsize=None)
def td_case(K, T, lens, seed=0):
    rng = np.random.RandomState(1000 * K + T + seed)
    est = rng.standard_normal((len(lens), K, T)).astype(np.float32)
    tgt = rng.standard_normal((len(lens), K, T)).astype(np.float32)
    W = rng.standard_normal((len(lens), K * K + 4 * K))
    for a in (est, tgt, W):
        a.setflags(write=False)
    return est, tgt, W


def td_stats_vector(q):
    """``pair_stats``' dictionary in the kernel's layout ``Set[K][K] | See | Stt | Se | St`` per example."""
    return torch.cat([q['set'].flatten(1), q['see'], q['stt'], q['se'], q['st']], dim=1)


def td_run(e, t, lens, W):
    """``pair_stats`` and the backward of ``(stats * W).sum()``; ``e`` and ``t`` are differentiable leaves or views of them."""
    from padertorch_amd.ops.losses import regression as R
    q = R.pair_stats(e, t, None if lens is None else list(lens))
    s = td_stats_vector(q)
    assert s.dtype == torch.float64
    (s * dev(W)).sum().backward()
    return s.detach(), q['n']


def td_assert_stats(s, n_got, est, tgt, lens):
    """The five sums against numpy fp64 sums.  Products of fp32 values are exact in fp64 and the kernel accumulates in fp64, so the only
    error is that of adding n terms in some order: at most ``n * 2^-52 * sum |terms|`` per statistic, n the number of samples summed
    (any order of n - 1 additions stays below (n - 1) * 2^-53 * sum |terms| to first order; the reference's own additions are
    counted too).  The gate is 4 x that."""
    B, K, T = est.shape
    s = s.cpu().numpy()
    for b in range(B):
        n = min(lens[b], T)
        assert n_got[b].item() == n
        e, t = est[b, :, :n].astype(np.float64), tgt[b, :, :n].astype(np.float64)
        want = np.concatenate([(e[:, None, :] * t[None, :, :]).sum(-1).ravel(), (e * e).sum(-1), (t * t).sum(-1), e.sum(-1), t.sum(-1)])
        mag = np.concatenate([(np.abs(e)[:, None, :] * np.abs(t)[None, :, :]).sum(-1).ravel(), (e * e).sum(-1), (t * t).sum(-1),
                              np.abs(e).sum(-1), np.abs(t).sum(-1)])
        err = np.abs(s[b] - want)
        assert (err <= 4 * n * 2. ** -52 * mag).all(), (b, float((err / (n * 2. ** -52 * mag)).max()))


def td_assert_grads(ge, gt, est, tgt, lens, W):
    """``d e_i = 2 W_see,i e_i + sum_j W_set,ij t_j + W_se,i`` (and symmetrically for the target) in fp64.  The kernel evaluates K + 2
    fp32 fused multiply-adds per sample with coefficients rounded to fp32; the gate is elementwise
    ``(K + 4) * 2^-23 * (|a| |x| + sum_j |b_j| |y_j| + |c|)``, and exactly zero at and beyond each length."""
    B, K, T = est.shape
    kk = K * K
    Wset = W[:, :kk].reshape(B, K, K)
    Wsee, Wstt, Wse, Wst = (W[:, kk + i * K:kk + (i + 1) * K] for i in range(4))
    e, t = est.astype(np.float64), tgt.astype(np.float64)
    for got, x, y, a, bm, c in ((ge, e, t, 2 * Wsee, Wset, Wse), (gt, t, e, 2 * Wstt, Wset.transpose(0, 2, 1), Wst)):
        got = got.cpu().numpy()
        assert got.shape == (B, K, T) and got.dtype == np.float32
        want = a[:, :, None] * x + np.einsum('bij,bjt->bit', bm, y) + c[:, :, None]
        bound = (K + 4) * 2. ** -23 * (np.abs(a)[:, :, None] * np.abs(x) + np.einsum('bij,bjt->bit', np.abs(bm), np.abs(y))
                                       + np.abs(c)[:, :, None])
        for b in range(B):
            n = min(lens[b], T)
            err = np.abs(got[b, :, :n] - want[b, :, :n])
            assert (err <= bound[b, :, :n]).all(), (b, float((err / bound[b, :, :n]).max()))
            assert not got[b, :, n:].any()


@pytest.mark.parametrize('T', [2052, 1027, 3])
@pytest.mark.parametrize('K', range(1, 9))
def test_td_statistics_and_gradient_vs_fp64(K, T):
    """``Set``, ``See``, ``Stt``, ``Se``, ``St`` of ``pair_stats`` and the gradient of a random fp64 weighting of them, K = 1..8 (1..4:
    ``td_stats_kernel<K>``, 5..8: ``td_stats_row_kernel``; ``td_lincomb_kernel<K>``), with lengths.  ``pick_chunk`` gives 1024-sample
    chunks at these sizes.  T = 2052 makes ``A.vec`` / ``P.vec`` true (lengths 1025, 1023, 5, 1 are no multiple of 4: the ragged tail
    of the float4 loop), T = 1027 and T = 3 make them false.  Bounds: ``td_assert_stats`` and ``td_assert_grads``."""
    lens = TD_LENS[T]
    est, tgt, W = td_case(K, T, lens)
    e, t = dev(est).requires_grad_(True), dev(tgt).requires_grad_(True)
    s, n = td_run(e, t, lens, W)
    td_assert_stats(s, n, est, tgt, lens)
    td_assert_grads(e.grad, t.grad, est, tgt, lens, W)


@pytest.mark.parametrize('K', [3, 6])
def test_td_views(K):
    """``big[:, :, 4:4 + T]`` (16-byte aligned, non-packed strides: float4 path) and ``big[:, :, 3:3 + T]`` (unaligned: scalar path),
    also with only one of estimate and target unaligned; NaN outside the views.  Calls that take the same path are bitwise equal -
    aligned views and the contiguous call, the three scalar calls among themselves - and every call stays within the bounds of
    ``td_assert_stats`` and ``td_assert_grads``."""
    T, lens = 1028, (1028, 1025, 1024, 1023, 7)
    est, tgt, W = td_case(K, T, lens)

    def view(a, off):
        big = torch.full(a.shape[:2] + (T + 8,), float('nan'), device=DEV)
        big[:, :, off:off + T] = dev(a)
        big.requires_grad_(True)
        return big, big[:, :, off:off + T]

    def run(oe, ot):
        (be, e), (bt, t) = view(est, oe), view(tgt, ot)
        assert e.stride() == (K * (T + 8), T + 8, 1)
        s, n = td_run(e, t, lens, W)
        ge, gt = be.grad[:, :, oe:oe + T], bt.grad[:, :, ot:ot + T]
        td_assert_stats(s, n, est, tgt, lens)
        td_assert_grads(ge, gt, est, tgt, lens, W)
        for big, off in ((be, oe), (bt, ot)):
            assert not big.grad[:, :, :off].any() and not big.grad[:, :, off + T:].any()
        return s, ge, gt
    e0, t0 = dev(est).requires_grad_(True), dev(tgt).requires_grad_(True)
    s0, n0 = td_run(e0, t0, lens, W)
    td_assert_stats(s0, n0, est, tgt, lens)
    td_assert_grads(e0.grad, t0.grad, est, tgt, lens, W)
    for a, b in zip(run(4, 4), (s0, e0.grad, t0.grad)):          # float4 path, like the contiguous call
        assert torch.equal(a, b)
    scalar = run(3, 3)
    for other in (run(3, 4), run(4, 3)):                          # one unaligned operand puts the whole call on the scalar path
        for a, b in zip(other, scalar):
            assert torch.equal(a, b)


@pytest.mark.parametrize('T', [2052, 1027])
@pytest.mark.parametrize('K', [2, 6])
def test_td_poisoned_tails(K, T):
    """NaN, then 1e30, at and beyond each length in both signals (K = 2: ``td_stats_kernel<2>``, K = 6: ``td_stats_row_kernel``; float4
    and scalar paths): statistics and gradients are bitwise the clean run."""
    lens = TD_LENS[T]
    est, tgt, W = td_case(K, T, lens)

    def run(poison):
        e, t = dev(est), dev(tgt)
        if poison is not None:
            for b, l in enumerate(lens):
                e[b, :, l:] = poison
                t[b, :, l:] = poison
        e.requires_grad_(True)
        t.requires_grad_(True)
        s, _ = td_run(e, t, lens, W)
        return s, e.grad, t.grad
    clean = run(None)
    for poison in POISONS:
        for a, b in zip(run(poison), clean):
            assert torch.equal(a, b)


def test_td_pit_losses_six_sources_end_to_end():
    """``pit_td_losses`` at K = 6 with ragged lengths: SI-SDR and log-MSE values, permutations (exact, under the candidate-gap
    condition) and gradients against torch fp64 autograd of the oracle's formulas (``losses_np.td_si_sdr_loss`` /
    ``td_log_mse_loss``) restated in torch on the CPU; gradients through ``close_grad`` of ``test_gpu_td`` (2e-4 of the largest
    entry)."""
    from padertorch_amd.ops.losses import regression as R
    rng = np.random.RandomState(6)
    B, K, T = 3, 6, 1500
    lens = (1500, 1025, 300)
    tgt = rng.standard_normal((B, K, T)).astype(np.float32)
    est = (tgt[:, ::-1] * 0.7 + 0.2 * rng.standard_normal((B, K, T))).astype(np.float32)

    def si_sdr_rows(e, t):                 # losses_np.td_si_sdr_loss before its reduction
        alpha = (e * t).sum(-1, keepdim=True) / (t * t).sum(-1, keepdim=True)
        s = alpha * t
        return -10 * torch.log10((s * s).sum(-1) / ((e - s) ** 2).sum(-1))

    def log_mse_rows(e, t):                # losses_np.td_log_mse_loss before its reduction
        return torch.log10(((e - t) ** 2).mean(-1))
    oracle = {'si-sdr': (si_sdr_rows, losses_np.td_si_sdr_loss, 'mean'), 'log-mse': (log_mse_rows, losses_np.td_log_mse_loss, 'sum')}
    for name, (rows, ofn, reduction) in oracle.items():
        x = dev(est).requires_grad_(True)
        loss, perm = R.pit_td_losses(x, dev(tgt), list(lens))[name]
        loss.sum().backward()
        xt = cpu64(est).requires_grad_(True)
        tot = 0
        for b, n in enumerate(lens):
            e, t = est[b, :, :n].astype(np.float64), tgt[b, :, :n].astype(np.float64)
            L = np.array([[ofn(e[i:i + 1], t[j:j + 1], reduction='sum') for j in range(K)] for i in range(K)])
            best, p, gap = walk_permutations(L)
            assert gap >= GAP, (name, b, gap)
            assert perm[b].tolist() == p, (name, b)
            r = rows(xt[b, p, :n], torch.from_numpy(t))
            value = r.mean() if reduction == 'mean' else r.sum()
            np.testing.assert_allclose(value.item(), best if reduction == 'mean' else best * K, rtol=1e-12, atol=1e-12)
            np.testing.assert_allclose(loss[b].item(), value.item(), rtol=1e-5, atol=1e-5)
            tot = tot + value
        tot.backward()
        close_grad(x.grad, xt.grad.numpy())
        for b, n in enumerate(lens):
            assert not x.grad[b, :, n:].any()
