"""The OR-PIT kernels (csrc/orpit.hip) against fp64 restatements written here with numpy / torch on the CPU.

Gates: statistics 1e-6 relative to max|want|; the fp32 gradient rows of the linear combination 1e-5 max|want|; flag head values 1e-5
max|want|, its gradients 2e-4 max|want| (the project's gates, tests/test_gpu_tasnet.py).  Every comparison prints its ratio
diff / (gate max|want|) (run with -s).

Shapes chosen by reading csrc/orpit.hip: a statistics workgroup covers a chunk of 1024 samples with 256 threads x float4, so T = 1, 3
(below one quad), 64, 65 (one lane group and a tail), 1027 (a second chunk of 3 samples: the two-stage sum) and 4099 (five chunks, a
tail); K = 0 (no targets), 1, 3 and 8 (the largest; 36 Gram sums).  ``out[:, 1:2]`` is an estimate view with M = 1 and a batch stride
of two rows; odd T makes every second row misaligned (the scalar kernels).  The flag head's workgroup is 64 lanes x 4 waves over the
rows: A = 1 (three idle waves), 20, 33 (nine trips, the last ragged), N = 5 / 64, E = 1, 7 and 257 (odd: the scalar kernels; 257 is
five workgroups, the last with one live lane) and, for the float4 kernels, E = 64 (16 live lanes) and 260 (two workgroups, one live
lane in the second)."""
import itertools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

STATS, ROWS, VALUE, GRAD = 1e-6, 1e-5, 1e-5, 2e-4


def close(name, got, want, gate, scale=None):
    """``|got - want| <= gate * max|want|``; ``scale`` replaces ``max|want|`` where the wanted value is a difference of terms that cancel."""
    got = torch.as_tensor(got).detach().double().cpu().reshape(-1)
    want = torch.as_tensor(np.asarray(want)).double().reshape(-1)
    assert got.shape == want.shape, (name, got.shape, want.shape)
    scale = (float(want.abs().max()) if want.numel() else 0.) if scale is None else scale
    err, bound = float((got - want).abs().max()) if want.numel() else 0., gate * scale
    ratio = err / bound if bound > 0 else (0. if err == 0 else float('inf'))
    print(f'orpit ratio {name}: {ratio:.4f} of the gate {gate:g}')
    assert ratio <= 1.0, (name, ratio)
    return ratio


def signals(B, M, K, T, seed, layout):
    """``(est [B, M, T], tgt [B, K, T])`` on the GPU.  ``view``: est is ``out[:, 1:2]`` of a ``[B, 2, T]`` tensor (M == 1)."""
    gen = torch.Generator().manual_seed(seed)
    tgt = torch.randn(B, K, T, generator=gen).cuda()
    if layout == 'view':
        out = torch.randn(B, 2, T, generator=gen).cuda()
        return out[:, 1:2], tgt
    return torch.randn(B, M, T, generator=gen).cuda(), tgt


CONFIGS = [(M, K, T, layout) for K, T in itertools.product([0, 1, 3, 8], [1, 3, 64, 65, 1027, 4099]) for M, layout in [(2, 'plain'), (1, 'view')]]


@pytest.mark.parametrize('M,K,T,layout', CONFIGS, ids=lambda v: str(v))
def test_rect_stats_and_lincomb_against_fp64(M, K, T, layout):
    B = 3
    est, tgt = signals(B, M, K, T, 160 + K + T, layout)
    e, t = est.double().cpu(), tgt.double().cpu()
    stats, gram = torch.ops.ptmi.td_rect_stats(est, tgt if K else None, True)
    assert stats.shape == (B, M * K + M) and gram.shape == (B, K, K) and stats.dtype == gram.dtype == torch.float64
    close('C', stats[:, :M * K], torch.einsum('bmt,bkt->bmk', e, t), STATS)
    close('See', stats[:, M * K:], (e * e).sum(-1), STATS)
    close('Gram', gram, torch.einsum('bjt,blt->bjl', t, t), STATS)
    assert torch.equal(gram, gram.transpose(1, 2))
    again, none = torch.ops.ptmi.td_rect_stats(est, tgt if K else None, False)
    assert torch.equal(again, stats) and none.numel() == 0                             # two runs are bit-identical
    gen = torch.Generator().manual_seed(T)
    g, a, bmat = torch.randn(B, generator=gen), torch.randn(B, M, generator=gen), torch.randn(B, M, K, generator=gen)
    out = torch.ops.ptmi.td_rect_lincomb(est, tgt if K else None, g.cuda(), a.cuda(), bmat.cuda())
    want = g.double()[:, None, None] * (a.double()[:, :, None] * e + torch.einsum('bmk,bkt->bmt', bmat.double(), t))
    close('lincomb', out, want, ROWS)
    assert torch.equal(out, torch.ops.ptmi.td_rect_lincomb(est, tgt if K else None, g.cuda(), a.cuda(), bmat.cuda()))
    ones = torch.ops.ptmi.td_rect_lincomb(est, tgt if K else None, None, a.cuda(), bmat.cuda())
    close('lincomb without g', ones, want / g.double()[:, None, None], ROWS)


@pytest.mark.parametrize('T', [57, 1027])
def test_rect_kernels_on_misaligned_rows(T):
    """Odd-T row views one float into their storage: the scalar kernels give the vector kernels' results, the sentinels stay."""
    B, K = 2, 3
    gen = torch.Generator().manual_seed(T)
    store_e, store_t = torch.full((B * 2 * T + 1,), 7.).cuda(), torch.full((B * K * T + 1,), 7.).cuda()
    est, tgt = store_e[1:].view(B, 2, T), store_t[1:].view(B, K, T)
    est.copy_(torch.randn(B, 2, T, generator=gen))
    tgt.copy_(torch.randn(B, K, T, generator=gen))
    stats, gram = torch.ops.ptmi.td_rect_stats(est, tgt, True)
    e, t = est.double().cpu(), tgt.double().cpu()
    close('C misaligned', stats[:, :2 * K], torch.einsum('bmt,bkt->bmk', e, t), STATS)
    close('Gram misaligned', gram, torch.einsum('bjt,blt->bjl', t, t), STATS)
    a, bmat = torch.randn(B, 2, generator=gen).cuda(), torch.randn(B, 2, K, generator=gen).cuda()
    out = torch.ops.ptmi.td_rect_lincomb(est, tgt, None, a, bmat)
    assert torch.equal(out, torch.ops.ptmi.td_rect_lincomb(est.clone(), tgt.clone(), None, a, bmat))
    assert float(store_e[0]) == 7. and float(store_t[0]) == 7.


# ------------------------------------------------------------------------------------------------ selection
def select_fp64(e, t, alive):
    """The reference's function on the alive targets of one example, in numpy fp64: (loss, choice, a [2], bmat [2, K])."""
    K, n = t.shape[0], e.shape[1]
    live = [j for j in range(K) if alive[j]]
    R, ln10 = len(live), np.log(10.)
    a, bmat = np.zeros(2), np.zeros((2, K))
    sse = lambda x: float((x * x).sum())      # noqa: E731
    if R >= 2:
        cand = []
        for i in live:
            rest = sum(t[j] for j in live if j != i)
            cand.append(np.log10(sse(e[0] - t[i]) / n) + np.log10(sse(e[1] - rest) / n) / (R - 1))
        i = live[int(np.argmin(cand))]
        others = [j for j in live if j != i]
        a[0], a[1] = 2 / (ln10 * sse(e[0] - t[i])), 2 / ((R - 1) * ln10 * sse(e[1] - sum(t[j] for j in others)))
        bmat[0, i], bmat[1, others] = -a[0], -a[1]
        return min(cand), i, a, bmat
    if R == 1:
        i = live[0]
        a[0], a[1] = 2 / (ln10 * sse(e[0] - t[i])), 2 / (ln10 * sse(e[1]))
        bmat[0, i] = -a[0]
        return np.log10(sse(e[0] - t[i]) / n) + np.log10(sse(e[1]) / n), i, a, bmat
    a[0], a[1] = 2 / (ln10 * sse(e[0])), 2 / (ln10 * sse(e[1]))
    return np.log10(sse(e[0]) / n) + np.log10(sse(e[1]) / n), -1, a, bmat


@pytest.mark.parametrize('K,T', [(0, 57), (1, 57), (2, 64), (4, 57), (8, 1027)], ids=str)
def test_selection_chain_against_fp64(K, T):
    """Every R from K down to 0 (and once more at 0) on a chain of launches; the alive masks after every launch."""
    B = 3
    gen = torch.Generator().manual_seed(K)
    tgt = (torch.randn(B, K, T, generator=gen) * (0.5 + torch.rand(B, K, 1, generator=gen))).cuda()
    alive = torch.ones((B, K), dtype=torch.int32, device='cuda')
    want_alive = np.ones((B, K), dtype=bool)
    gram = None
    for step in range(K + 2):
        est = torch.randn(B, 2, T, generator=gen).cuda()
        stats, new = torch.ops.ptmi.td_rect_stats(est, tgt if K else None, gram is None)
        gram = new if gram is None else gram
        loss, choice, alive, a, bmat = torch.ops.ptmi.orpit_select(stats, gram, alive, T)
        for b in range(B):
            w_loss, w_choice, w_a, w_b = select_fp64(est[b].double().cpu().numpy(), tgt[b].double().cpu().numpy(), want_alive[b])
            assert int(choice[b]) == w_choice, (step, b)
            assert abs(float(loss[b]) - w_loss) <= 1e-5 * max(1., abs(w_loss)), (step, b, float(loss[b]), w_loss)
            close(f'a step {step} example {b}', a[b], w_a, ROWS)
            close(f'bmat step {step} example {b}', bmat[b], w_b, ROWS)
            if w_choice >= 0:
                want_alive[b, w_choice] = False
        assert np.array_equal(alive.cpu().numpy().astype(bool), want_alive), step
    assert not want_alive.any()


def test_selection_tie_picks_the_lower_index():
    gen = torch.Generator().manual_seed(3)
    tgt = torch.randn(2, 4, 65, generator=gen)
    tgt[0, 3] = tgt[0, 1]                                                           # example 0: targets 1 and 3 are the same signal
    tgt[1, 2] = tgt[1, 0]
    est = torch.stack([torch.stack([tgt[0, 1] + 0.01, tgt[0].sum(0) - tgt[0, 1]]), torch.stack([tgt[1, 0] - 0.02, tgt[1].sum(0) - tgt[1, 0]])])
    stats, gram = torch.ops.ptmi.td_rect_stats(est.cuda(), tgt.cuda(), True)
    alive = torch.ones((2, 4), dtype=torch.int32, device='cuda')
    _, choice, alive, _, _ = torch.ops.ptmi.orpit_select(stats, gram, alive, 65)
    assert choice.tolist() == [1, 0] and alive.tolist() == [[1, 0, 1, 1], [0, 1, 1, 1]]


def test_iterations_gradient_and_nan_isolation():
    """``or_pit_iterations`` under autograd against torch's own fp64 graph of the same closed choice; a NaN stays in its example."""
    from padertorch_amd.ops import orpit
    B, K, T = 3, 3, 203
    gen = torch.Generator().manual_seed(11)
    tgt = torch.randn(B, K, T, generator=gen) * (0.5 + torch.rand(B, K, 1, generator=gen))
    ests = [torch.randn(B, 2, T, generator=gen) for _ in range(3)]
    leaves = [e.cuda().requires_grad_() for e in ests]
    losses, choices = orpit.or_pit_iterations(leaves, tgt.cuda())
    weight = torch.randn(3, B, generator=gen)
    grads = torch.autograd.grad((losses * weight.cuda()).sum(), leaves)
    alive = np.ones((B, K), dtype=bool)
    for k in range(3):
        e64 = ests[k].double().requires_grad_()
        total = 0
        for b in range(B):
            _, i, _, _ = select_fp64(ests[k][b].double().numpy(), tgt[b].double().numpy(), alive[b])
            others = [j for j in range(K) if alive[b, j] and j != i]
            rest = tgt[b, others].double().sum(0) if others else torch.zeros(T, dtype=torch.float64)
            w1 = 1 / max(len(others), 1)
            loss = torch.log10(((e64[b, 0] - tgt[b, i].double()) ** 2).mean()) + w1 * torch.log10(((e64[b, 1] - rest) ** 2).mean())
            assert int(choices[k, b]) == i and abs(float(losses[k, b]) - float(loss)) <= 1e-5 * max(1., abs(float(loss)))
            total = total + weight[k, b].double() * loss
            alive[b, i] = False
        close(f'd estimate of iteration {k}', grads[k], torch.autograd.grad(total, e64)[0], ROWS)
    again, _ = orpit.or_pit_iterations(leaves, tgt.cuda())
    assert torch.equal(again, losses)
    bad = [e.detach().clone() for e in leaves]
    bad[0][1, 0, 40] = float('nan')
    nan_losses, _ = orpit.or_pit_iterations(bad, tgt.cuda())
    assert bool(torch.isnan(nan_losses[0, 1])) and bool(torch.isfinite(nan_losses[:, [0, 2]]).all()) and bool(torch.isfinite(nan_losses[1:]).all())
    with pytest.raises(ValueError, match='no gradient'):
        orpit.or_pit_iterations(leaves, tgt.cuda().requires_grad_())


# ------------------------------------------------------------------------------------------------ flag head
def flag_fp64(additional, weight, bias, mode, mask, encoded):
    pre = torch.einsum('bae,a->be', additional, weight.reshape(-1)) + bias.reshape(())
    if mode == 'mean':
        return torch.sigmoid(pre.mean(1)), pre
    k = 1 if mode == 'res-weighted-mean' else 0
    estimate = mask[k] * encoded if encoded is not None else mask[k]
    w = (estimate ** 2).mean(1)
    return torch.sigmoid((pre * w).sum(1) / w.sum(1)), pre


def cancelled_scales(ref, mode, with_encoded, flag, pre, gflag):
    """With ONE frame the weights cancel (``pre w / w``): the derivative w.r.t. mask and encoded is exactly zero, the difference of two
    equal terms ``gx pre / den * dw`` and ``gx x / den * dw``.  ``max|want|`` is then zero (or fp64 rounding) and no scale; the gate is taken
    relative to the magnitude of ONE of the cancelling terms, which is what fp32 rounding of ``pre`` is relative to."""
    with torch.no_grad():
        mask = ref[3][1 if mode == 'res-weighted-mean' else 0]
        enc = ref[4] if with_encoded else torch.ones_like(mask)
        den = ((mask * enc) ** 2).mean(1).sum(1)
        term = (gflag.double() * flag * (1 - flag)).abs()[:, None] * pre.abs() / den[:, None] * 2 / mask.shape[1]      # [B, E]
        return dict(mask=float((term[:, None] * mask.abs() * enc ** 2).max()), encoded=float((term[:, None] * mask ** 2 * enc.abs()).max()))


@pytest.mark.parametrize('with_encoded', [True, False], ids=['encoded', 'null'])
@pytest.mark.parametrize('mode', ['mean', 'res-weighted-mean', 'est-weighted-mean'])
@pytest.mark.parametrize('A,N,E', list(itertools.product([1, 20, 33], [5, 64], [1, 7, 257])) + [(20, 64, 260), (33, 5, 64)], ids=str)
def test_flag_head_against_fp64(A, N, E, mode, with_encoded):
    from padertorch_amd.ops import orpit
    B, K = 2, 2
    gen = torch.Generator().manual_seed(A + N + E)
    host = [torch.randn(B, A, E, generator=gen), torch.randn(1, A, generator=gen) * 0.3, torch.randn(1, generator=gen),
            torch.rand(K, B, N, E, generator=gen), torch.randn(B, N, E, generator=gen)]
    if not with_encoded:
        host = host[:4]
    gflag, gpre = torch.randn(B, generator=gen), torch.randn(B, E, generator=gen)
    dev = [h.cuda().requires_grad_() for h in host]
    ref = [h.double().requires_grad_() for h in host]
    flag, pre = orpit.flag_head(dev[0], dev[1], dev[2], mode, dev[3], dev[4] if with_encoded else None)
    want_flag, want_pre = flag_fp64(ref[0], ref[1], ref[2], mode, ref[3], ref[4] if with_encoded else None)
    assert flag.shape == (B,) and pre.shape == (B, E)
    close('flag', flag, want_flag.detach(), VALUE)
    close('pre', pre, want_pre.detach(), VALUE)
    used = len(host) if mode != 'mean' else 3
    got = torch.autograd.grad((flag * gflag.cuda()).sum() + (pre * gpre.cuda()).sum(), dev[:used], retain_graph=True)
    want = torch.autograd.grad((want_flag * gflag.double()).sum() + (want_pre * gpre.double()).sum(), ref[:used])
    scales = cancelled_scales(ref, mode, with_encoded, want_flag, want_pre, gflag) if E == 1 and mode != 'mean' else {}
    for name, g, w in zip(['additional', 'weight', 'bias', 'mask', 'encoded'], got, want):
        assert g.shape == w.shape
        close(f'd {name}', g, w, GRAD, scales.get(name))
    only_flag = torch.autograd.grad(flag.sum(), dev[:used], retain_graph=True)                      # pre gets no gradient: the NULL path
    want_only = torch.autograd.grad(flag_fp64(ref[0], ref[1], ref[2], mode, ref[3], ref[4] if with_encoded else None)[0].sum(), ref[:used])
    for name, g, w in zip(['additional', 'weight', 'bias', 'mask', 'encoded'], only_flag, want_only):
        close(f'd {name} (flag alone)', g, w, GRAD, scales.get(name))
    flag2, pre2 = orpit.flag_head(dev[0], dev[1], dev[2], mode, dev[3], dev[4] if with_encoded else None)
    assert torch.equal(flag2, flag) and torch.equal(pre2, pre)
    again = torch.autograd.grad((flag2 * gflag.cuda()).sum() + (pre2 * gpre.cuda()).sum(), dev[:used])
    for a, b in zip(again, got):
        assert torch.equal(a, b)


def test_flag_head_silent_stream_and_nan_isolation():
    from padertorch_amd.ops import orpit
    gen = torch.Generator().manual_seed(5)
    additional, weight, bias = torch.randn(2, 4, 9, generator=gen).cuda(), torch.randn(4, generator=gen).cuda(), torch.zeros(1).cuda()
    mask, encoded = torch.rand(2, 2, 3, 9, generator=gen).cuda(), torch.randn(2, 3, 9, generator=gen).cuda()
    encoded[1] = 0                                                                       # a silent stream: 0 / 0, no epsilon
    flag, _ = orpit.flag_head(additional, weight, bias, 'res-weighted-mean', mask, encoded)
    assert bool(torch.isfinite(flag[0])) and bool(torch.isnan(flag[1]))
    additional[0, 1, 2] = float('nan')
    flag, pre = orpit.flag_head(additional, weight, bias, 'mean')
    assert bool(torch.isnan(flag[0])) and bool(torch.isfinite(flag[1])) and bool(torch.isfinite(pre[1]).all())


def test_other_dtypes_and_cpu_tensors_are_refused():
    from padertorch_amd.ops import orpit
    from padertorch_amd.ops.losses import log_mse_loss, one_and_rest_permutation_invariant_loss
    x = torch.zeros(2, 3, 8, device='cuda')
    with pytest.raises(NotImplementedError, match='float32'):
        orpit.flag_head(x.double(), torch.ones(3, device='cuda'), torch.ones(1, device='cuda'))
    with pytest.raises(NotImplementedError, match='float32'):
        orpit.or_pit_iterations([x.half()], x)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        orpit.flag_head(x.cpu(), torch.ones(3), torch.ones(1))
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        orpit.or_pit_iterations([x.cpu()[:, :2]], x.cpu())
    with pytest.raises(NotImplementedError):
        torch.ops.ptmi.orpit_flag_forward(x.cpu(), torch.ones(3), torch.ones(1), None, None, 0)
    with pytest.raises(NotImplementedError, match='no loss'):
        one_and_rest_permutation_invariant_loss(x[0, :2], x[0], lambda a, b: (a - b).sum(), True)
    with pytest.raises(ValueError, match='mode'):
        orpit.flag_head(x, torch.ones(3, device='cuda'), torch.ones(1, device='cuda'), 'min')
    assert callable(log_mse_loss)
