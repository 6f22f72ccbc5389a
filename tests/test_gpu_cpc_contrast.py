"""The fused contrast of CPC (``csrc/cpc_contrast.hip``, ``ops.cpc_contrast.contrastive_scores``) against a plain fp64 restatement of
``contrib/mk/modules/contrastive.py:343-471`` plus ``CrossEntropyLoss`` / ``argmax`` / the ``> -inf`` count, dense torch ops on the CPU.

The gates are four times the largest error of the SAME restatement run in fp32 on the CPU against its fp64 run over these cases, relative
to the largest magnitude of the quantity in the case (``scripts/cpc_contrast_gates.py``, ``profiles/cpc_contrast_gates.txt``)."""
import math

import pytest
import torch
import torch.nn.functional as F

from padertorch_amd.ops.cpc_contrast import kCpcBM, kCpcBN

pytestmark = pytest.mark.gpu

#: profiles/cpc_contrast_gates.txt: 4 x the fp32 restatement's largest relative error per quantity
GATES = {'ce': 1.0e-5, 'dz_hat': 1.5e-5, 'dz': 1.5e-5, 'logits': 1.4e-6}
TEMPERATURE = 4.

#: (b, d, t, steps, dist) for 'time' and 'all': one entry with d no multiple of 4 and no mask | the key tile's edge 32 + 8, step 0, both
#: signs, band mask, wrapped keys | T_s across the owned tile | d across the 128-feature chunk
SHAPES = [(1, 5, 9, (1,), 0), (3, 24, 40, (-3, 0, 2, 5), 3), (2, 70, kCpcBM + 3, (-2, 1), 2), (2, 130, 3 * kCpcBN + 1, (3,), 4)]
#: (b, labels, invert_batch_mask) for 'batch' (d = 12, t = 19: three tiles of 8 positions, steps (-2, 1, 3)): the smallest batch | duplicate
#: labels | the batch across a 16-row tile with the inverted mask
BATCHES = [(2, None, False), (5, (0, 1, 0, 2, 1), False), (17, tuple(int(i >= 13) for i in range(17)), True)]
CASES = [(m, *s, None, False, 1.) for m in ('time', 'all') for s in SHAPES] + \
        [('batch', b, 12, 19, (-2, 1, 3), 0, lab, inv, r) for b, lab, inv in BATCHES for r in (1., 0.5)]


def inputs(b, d, t, steps, dtype=torch.float64):
    g = torch.Generator().manual_seed(1000 * b + t)
    z = torch.randn(b, d, t, generator=g, dtype=torch.float64)
    z_hat = torch.cat([0.5 * torch.roll(z, -s, 2) + torch.randn(b, d, t, generator=g, dtype=torch.float64) for s in steps], 1)
    gout = [torch.randn(b, t - abs(s), generator=g, dtype=torch.float64).to(dtype) for s in steps]
    return z_hat.to(dtype), z.to(dtype), gout


def log_batch_mask(b, labels, invert, dtype=torch.float64):
    """contrastive.py:350-368."""
    if labels is None:
        return torch.zeros(b, b, dtype=dtype)
    labels = torch.tensor(labels)
    mask = labels[:, None] != labels[None, :]
    mask = (~mask).to(dtype) if invert else mask.to(dtype) + torch.eye(b, dtype=dtype)
    return torch.log(mask)


def restatement(z_hat, z, gout, mode, steps, dist, lbm, ratio):
    """``(per step (logits [b, K, T_s], ce, hits, finite), dz_hat, dz)`` in the dtype of ``z``."""
    b, d, t = z.shape
    z_hat, z = z_hat.clone().requires_grad_(True), z.clone().requires_grad_(True)
    out, loss = [], 0.
    for n, s in enumerate(steps):
        Ts, qoff, sh = t - abs(s), max(-s, 0), max(s, 0)
        q = z_hat[:, n * d:(n + 1) * d, qoff:qoff + Ts]
        if mode == 'batch':
            sim = torch.einsum('idt,jdt->tij', q, z[:, :, sh:sh + Ts]) / TEMPERATURE + lbm[None]
            kk = max(int(math.ceil(b * (1 - ratio))), 1)
            th = torch.topk(sim, kk, dim=2).values.min(2).values[..., None]
            keep = (sim <= th) | torch.eye(b, dtype=torch.bool)[None]
            logits = (sim + keep.to(sim.dtype).log()).permute(1, 2, 0)
            targets = torch.arange(b)[:, None].expand(b, Ts)
        else:
            keys = torch.roll(z, -sh, 2)
            band = (torch.arange(t)[:, None] - torch.arange(Ts)[None]).abs()
            band = (band <= dist - 1) & (band > 0) if dist > 1 else torch.zeros(t, Ts, dtype=torch.bool)
            if mode == 'time':
                logits = torch.einsum('idq,idk->ikq', q, keys) / TEMPERATURE
                logits = torch.where(band[None], -math.inf, logits)
                targets = torch.arange(Ts)[None].expand(b, Ts)
            else:
                logits = torch.einsum('idq,jdk->ijkq', q, keys) / TEMPERATURE
                logits = torch.where(torch.eye(b, dtype=torch.bool)[:, :, None, None] & band, -math.inf, logits).reshape(b, b * t, Ts)
                targets = torch.arange(b)[:, None] * t + torch.arange(Ts)[None]
        ce = F.cross_entropy(logits, targets, reduction='none')
        loss = loss + (ce * gout[n]).sum()
        out.append((logits.detach(), ce.detach(), (logits.argmax(1) == targets).to(z.dtype), (logits > -math.inf).sum(1)))
    loss.backward()
    return out, z_hat.grad, z.grad


def rel(got, want):
    return float((got.double().cpu() - want).abs().max() / want.abs().max())


def run(z_hat, z, gout, mode, steps, dist, lbm, ratio, dense=True):
    from padertorch_amd.ops.cpc_contrast import contrastive_scores
    z_hat, z = z_hat.float().cuda().requires_grad_(True), z.float().cuda().requires_grad_(True)
    stats = contrastive_scores(z_hat, z, steps, mode, TEMPERATURE, dist, None if lbm is None else lbm.float().cuda(), ratio, dense=dense)
    sum((st.ce * g.float().cuda()).sum() for st, g in zip(stats, gout)).backward()
    return stats, z_hat.grad, z.grad


@pytest.mark.parametrize('case', CASES, ids=lambda c: '-'.join(str(v).replace(' ', '') for v in c[:5]) + f'-{c[8]}')
def test_against_fp64(case):
    mode, b, d, t, steps, dist, labels, invert, ratio = case
    z_hat, z, gout = inputs(b, d, t, steps)
    lbm = log_batch_mask(b, labels, invert) if mode == 'batch' else None
    want, want_dzh, want_dz = restatement(z_hat, z, gout, mode, steps, dist, lbm, ratio)
    got, got_dzh, got_dz = run(z_hat, z, gout, mode, steps, dist, lbm, ratio)
    errors = {'dz_hat': rel(got_dzh, want_dzh), 'dz': rel(got_dz, want_dz), 'ce': 0., 'logits': 0.}
    top = max(float(w[0][w[0] > -math.inf].abs().max()) for w in want)
    ce_top = max(float(w[1].abs().max()) for w in want)
    compared = excluded = ref_hits = 0
    for st, (logits, ce, hits, finite) in zip(got, want):
        inf = logits == -math.inf
        assert torch.equal(st.logits.cpu() == -math.inf, inf)
        assert torch.equal(st.finite.cpu().long(), finite)
        errors['logits'] = max(errors['logits'], float((st.logits.cpu().double() - logits)[~inf].abs().max()) / top)
        errors['ce'] = max(errors['ce'], float((st.ce.detach().cpu().double() - ce).abs().max()) / ce_top)
        top2 = torch.topk(logits, 2, dim=1).values if logits.shape[1] > 1 else None
        clear = (top2[:, 0] - top2[:, 1] >= 1e-3 * top) if top2 is not None else torch.ones_like(hits, dtype=torch.bool)
        assert torch.equal(st.hits.cpu().double()[clear], hits[clear])
        compared, excluded, ref_hits = compared + hits.numel(), excluded + int((~clear).sum()), ref_hits + float(hits.sum())
    print(case, errors, f'hits: {excluded} of {compared} rows excluded, reference hit rate {ref_hits / compared:.3f}')
    assert excluded <= 0.05 * compared
    if b > 2:
        assert 0 < ref_hits < compared
    for k in GATES:
        assert errors[k] <= GATES[k], (k, errors)


def test_default_path_has_no_dense_logits_and_same_statistics():
    mode, (b, d, t, steps, dist) = 'all', SHAPES[1]
    z_hat, z, gout = inputs(b, d, t, steps)
    dense, sparse = run(z_hat, z, gout, mode, steps, dist, None, 1.), run(z_hat, z, gout, mode, steps, dist, None, 1., dense=False)
    assert all(st.logits is None for st in sparse[0])
    for a, c in zip(dense[0], sparse[0]):
        assert torch.equal(a.ce, c.ce) and torch.equal(a.hits, c.hits) and torch.equal(a.finite, c.finite)
    assert torch.equal(dense[1], sparse[1]) and torch.equal(dense[2], sparse[2])


def test_capture_replays_other_inputs_bit_identically():
    from padertorch_amd.ops.cpc_contrast import contrastive_scores
    b, d, t, steps, dist = SHAPES[1]
    z_hat, z, gout = (x.float().cuda() if torch.is_tensor(x) else [g.float().cuda() for g in x] for x in inputs(b, d, t, steps))
    other = [x.flip(0).contiguous() for x in (z_hat, z)]

    def step(zh_, z_):
        stats = contrastive_scores(zh_, z_, steps, 'all', TEMPERATURE, dist)
        loss = sum((st.ce * g).sum() for st, g in zip(stats, gout))
        return (loss, *torch.autograd.grad(loss, (zh_, z_)), *[st.hits for st in stats])
    eager = [x.clone() for x in step(*[x.clone().requires_grad_(True) for x in other])]
    zhs, zs = z_hat.clone().requires_grad_(True), z.clone().requires_grad_(True)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step(zhs, zs)                                       # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = step(zhs, zs)
    for _ in range(3):                                      # several replays: each equal to the eager call on those inputs
        with torch.no_grad():
            zhs.copy_(other[0])
            zs.copy_(other[1])
        graph.replay()
        torch.cuda.synchronize()
        for a, c in zip(out, eager):
            assert torch.equal(a, c)
