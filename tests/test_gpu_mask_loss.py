"""``ops.mask_bce_loss`` (``csrc/mask_loss.hip``) against the numpy fp64 restatement of tests/test_mask_loss_host.py on the same fp32
inputs, and ``MaskEstimatorModel`` against the reference's fp64 results (tests/golden/g19_mask_model.npz, made by
tests/golden/make_golden_mask_model.py from the real reference).

Gates: pooled and weighted losses 1e-5 relative, gradients |diff| <= 2e-4 max|want| elementwise, exact zeros behind the lengths; the
model's loss scalars 1e-4 relative, its gradients 2e-4 max|want|.  Inputs of a selecting reduction (median, min, max) are drawn so that
the selected loss is at least 1e-5 of its value away from its nearest unequal neighbour (``ref_gap``: a property of the input, judged by
the restatement alone) - closer, fp32 rounding may select another element than fp64 does, which is not what is tested.  Every
comparison prints its share of the gate (-s)."""
import functools
import json

import numpy as np
import pytest
import torch

from test_mask_loss_host import REDUCTIONS, build_model, load_g19, ref_gap, ref_mask_bce, tie_case

pytestmark = pytest.mark.gpu

VALUE, GRAD, SCALAR = 1e-5, 2e-4, 1e-4
DEV = 'cuda'

#: (B, C, T, F, num_frames, layout)
SHAPES = {
    'one': (1, 1, 1, 1, [1], 'dense'),
    'scalar': (3, 2, 7, 5, [7, 4, 1], 'estimator'),          # odd and even n_b
    'float4': (2, 2, 6, 8, [6, 3], 'estimator'),
    'misaligned': (2, 1, 5, 8, [5, 2], 'offset'),            # base pointer one float behind a 16-byte boundary
    'many': (2, 3, 300, 65, [300, 171], 'estimator'),        # one example over many workgroups
}


@pytest.fixture(scope='module')
def g19():
    return load_g19()


def share(name, got, want, gate, relative_to_max=True, floor=0.):
    """``floor``: an absolute allowance, for values fp32 cannot hold to a relative precision (below its smallest normal number)."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape, (name, got.shape, want.shape)
    bound = np.maximum(gate * (np.abs(want).max() if relative_to_max else np.abs(want)), floor)
    with np.errstate(all='ignore'):
        ratio = np.where(np.abs(got - want) == 0, 0., np.abs(got - want) / bound)
    ratio = float(np.max(ratio)) if ratio.size else 0.
    print(f'mask_loss ratio {name}: {ratio:.4f} of the gate {gate:g}')
    assert ratio <= 1.0, (name, ratio)
    return ratio


@functools.lru_cache(maxsize=None)
def drawn(shape, reduction):
    """Host inputs of a shape (float32 logits, targets, real and complex power, upstream gradients): the first seed whose selected
    losses keep their distance from their neighbours."""
    B, C, T, F, frames, _ = SHAPES[shape]
    seed = 1900
    while True:
        rng = np.random.RandomState(seed)
        logits = (rng.randn(B, C, T, F) * 2).astype(np.float32)
        target = rng.uniform(0, 1, (B, C, T, F)).astype(np.float32)
        if ref_gap(logits, target, frames, reduction) >= 1e-5:
            break
        seed += 1
    real = rng.uniform(0, 2, (B, C, T, F)).astype(np.float32)
    cplx = (rng.randn(B, C, T, F) + 1j * rng.randn(B, C, T, F)).astype(np.complex64)
    return logits, target, dict(none=None, real=real, complex=cplx), rng.randn(B).astype(np.float32), rng.randn(B).astype(np.float32)


def place(host, layout):
    """A host ``[B, C, T, F]`` array on the device: ``dense``; ``estimator``: the estimator's own view, ``out[..., :F]`` of a
    ``[C B, T, 2 F]`` buffer folded ``'(c b) t f -> b c t f'``; ``offset``: dense, one float behind an aligned base."""
    t = torch.from_numpy(host)
    B, C, T, F = t.shape
    if layout == 'estimator':
        buf = torch.full((C * B, T, 2 * F), float('nan'), dtype=t.dtype, device=DEV)
        view = buf.reshape(C, B, T, 2 * F).transpose(0, 1)[..., :F]
        view.copy_(t)
        assert not view.is_contiguous()
        return view
    if layout == 'offset':
        flat = torch.empty(t.numel() + 1, dtype=t.dtype, device=DEV)
        view = flat[1:].view(B, C, T, F)
        view.copy_(t)
        assert view.data_ptr() % 16 != 0
        return view
    return t.to(DEV)


def run_op(logits, target, frames, power, reduction, gp, gw):
    """The op and its backward on device tensors -> host ``(pooled, weighted, d logits)``."""
    from padertorch_amd import ops
    x = logits.detach().requires_grad_()
    pooled, weighted = ops.mask_bce_loss(x, target, frames, power, reduction)
    total = (pooled * gp).sum()
    if weighted is not None:
        total = total + (weighted * gw).sum()
    grad, = torch.autograd.grad(total, x)
    assert grad.shape == x.shape and grad.is_contiguous()
    return pooled.detach().cpu().numpy(), None if weighted is None else weighted.detach().cpu().numpy(), grad.cpu().numpy()


@pytest.mark.parametrize('power', ['none', 'real', 'complex'])
@pytest.mark.parametrize('reduction', REDUCTIONS)
@pytest.mark.parametrize('shape', list(SHAPES))
def test_op_against_the_restatement(shape, reduction, power):
    B, C, T, F, frames, layout = SHAPES[shape]
    logits, target, powers, gp, gw = drawn(shape, reduction)
    pw = powers[power]
    want = ref_mask_bce(logits, target, frames, pw, reduction, gp, gw)
    # behind the lengths the device inputs hold NaN: nothing there may be read
    poisoned = [a.copy() for a in (logits, target)] + [None if pw is None else pw.copy()]
    for a in poisoned:
        for b, n in enumerate(frames):
            if a is not None:
                a[b, :, n:] = np.nan
    got = run_op(place(poisoned[0], layout), place(poisoned[1], 'dense' if layout == 'estimator' else layout), frames,
                 None if pw is None else place(poisoned[2], 'dense' if layout == 'estimator' else layout), reduction,
                 torch.from_numpy(gp).to(DEV), torch.from_numpy(gw).to(DEV))
    share(f'{shape} {reduction} {power} pooled', got[0], want[0], VALUE, relative_to_max=False)
    if pw is None:
        assert got[1] is None
    else:
        share(f'{shape} {reduction} {power} weighted', got[1], want[1], VALUE, relative_to_max=False)
    share(f'{shape} {reduction} {power} d logits', got[2], want[2], GRAD)
    for b, n in enumerate(frames):
        assert not got[2][b, :, n:].any() and not np.signbit(got[2][b, :, n:]).any()
    if reduction != 'mean' and pw is None:
        assert (got[2] != 0).sum() == (want[2] != 0).sum() == B         # one selected element per example


def test_strided_targets_and_device_lengths():
    """The targets as the view a single padding call of ``[T_b, C, F]`` examples leaves (``[B, T, C, F]`` permuted), the lengths as an
    int32 device tensor."""
    B, C, T, F, frames, _ = SHAPES['float4']
    logits, target, powers, gp, gw = drawn('float4', 'median')
    want = ref_mask_bce(logits, target, frames, powers['complex'], 'median', gp, gw)
    tgt = torch.from_numpy(target).to(DEV).permute(0, 2, 1, 3).contiguous().permute(0, 2, 1, 3)
    assert not tgt.is_contiguous()
    got = run_op(place(logits, 'estimator'), tgt, torch.tensor(frames, dtype=torch.int32, device=DEV),
                 torch.from_numpy(powers['complex']).to(DEV), 'median', torch.from_numpy(gp).to(DEV), torch.from_numpy(gw).to(DEV))
    share('strided target pooled', got[0], want[0], VALUE, relative_to_max=False)
    share('strided target weighted', got[1], want[1], VALUE, relative_to_max=False)
    share('strided target d logits', got[2], want[2], GRAD)


@pytest.mark.parametrize('reduction', ['median', 'min', 'max'])
@pytest.mark.parametrize('n', [35, 36])
def test_ties_split_evenly(reduction, n):
    """The minimum, the maximum and the median are each attained by 3 duplicated (logit, target) pairs: the pooled value is that
    element, each of the three gets a third of the gradient, everything else exactly zero."""
    x, t, where = tie_case(np.random.RandomState(n), n)
    logits, target = x.reshape(1, 1, 1, n), t.reshape(1, 1, 1, n)
    want = ref_mask_bce(logits, target, [1], None, reduction, [1.5])
    got = run_op(torch.from_numpy(logits).to(DEV), torch.from_numpy(target).to(DEV), None, None, reduction,
                 torch.tensor([1.5], device=DEV), None)
    share(f'ties {reduction} pooled', got[0], want[0], 1e-6, relative_to_max=False)
    hit = np.flatnonzero(got[2])
    assert hit.tolist() == sorted(where[reduction].tolist()) and len(hit) == 3
    assert len({got[2].reshape(-1)[i].tobytes() for i in hit}) == 1                     # the same pair, the same third
    share(f'ties {reduction} d logits', got[2], want[2], GRAD)


def test_extreme_logits_are_finite():
    grid = np.array([[x, t] for x in (-200., 0., 200.) for t in (0., 1., 0.5)], np.float32)
    logits, target = grid[:, 0].reshape(1, 1, 3, 3), grid[:, 1].reshape(1, 1, 3, 3)
    for reduction in REDUCTIONS:
        want = ref_mask_bce(logits, target, [3], None, reduction, [1.])
        got = run_op(torch.from_numpy(logits).to(DEV), torch.from_numpy(target).to(DEV), [3], None, reduction,
                     torch.ones(1, device=DEV), None)
        assert np.isfinite(got[0]).all() and np.isfinite(got[2]).all()
        # (the smallest loss here is log1p(exp(-200)) = 1.4e-87 in fp64: below fp32's range, where it is 0)
        share(f'extreme {reduction} pooled', got[0], want[0], VALUE, relative_to_max=False, floor=float(np.finfo(np.float32).tiny))
        if reduction == 'mean':                 # (the selections have ties here: among 0 losses, and among 200 s)
            share(f'extreme {reduction} d logits', got[2], want[2], GRAD)


@pytest.mark.parametrize('reduction', REDUCTIONS)
def test_padding_has_no_influence_and_nan_inside_has(reduction):
    from padertorch_amd import ops
    B, C, T, F, frames, _ = SHAPES['scalar']
    logits, target, powers, gp, gw = drawn('scalar', reduction)
    dev = [torch.from_numpy(a).to(DEV) for a in (logits, target, powers['complex'], gp, gw)]
    clean = run_op(dev[0], dev[1], frames, dev[2], reduction, dev[3], dev[4])
    for fill in (float('nan'), 1e30):
        bad = [a.clone() for a in dev[:3]]
        for a in bad:
            for b, n in enumerate(frames):
                a[b, :, n:] = fill
        got = run_op(bad[0], bad[1], frames, bad[2], reduction, dev[3], dev[4])
        for a, b in zip(clean, got):
            assert a.tobytes() == b.tobytes(), fill
    inside = dev[0].clone()
    inside[1, 1, 2, 3] = float('nan')
    pooled, weighted = ops.mask_bce_loss(inside, dev[1], frames, dev[2], reduction)
    assert torch.isnan(pooled).tolist() == [False, True, False] and torch.isnan(weighted).tolist() == [False, True, False]
    assert torch.equal(pooled[[0, 2]].cpu(), torch.from_numpy(clean[0])[[0, 2]])


@pytest.mark.parametrize('reduction', ['median', 'min'])
def test_negative_losses(reduction):
    """Targets outside [0, 1] are legal input: with a target of 2 the loss of a positive logit is negative."""
    rng = np.random.RandomState(7)
    while True:
        logits = (np.abs(rng.randn(2, 1, 3, 7)) * 3 + 0.5).astype(np.float32)
        target = np.where(rng.rand(2, 1, 3, 7) < 0.8, 2., rng.rand(2, 1, 3, 7)).astype(np.float32)
        if ref_gap(logits, target, [3, 2], reduction) >= 1e-5:
            break
    want = ref_mask_bce(logits, target, [3, 2], None, reduction, [1., -2.])
    assert (want[0] < 0).all()
    got = run_op(torch.from_numpy(logits).to(DEV), torch.from_numpy(target).to(DEV), [3, 2], None, reduction,
                 torch.tensor([1., -2.], device=DEV), None)
    share(f'negative {reduction} pooled', got[0], want[0], VALUE, relative_to_max=False)
    share(f'negative {reduction} d logits', got[2], want[2], GRAD)


def test_zero_power_gives_nan_and_device_argument_errors():
    from padertorch_amd import ops
    x, t = torch.randn(2, 1, 3, 4, device=DEV), torch.rand(2, 1, 3, 4, device=DEV)
    w = torch.ones(2, 1, 3, 4, device=DEV)
    w[1] = 0
    pooled, weighted = ops.mask_bce_loss(x, t, None, w, 'mean')
    assert torch.isfinite(pooled).all() and torch.isnan(weighted).tolist() == [False, True]
    with pytest.raises(ValueError, match=r'mask_bce_loss.*unit stride'):
        ops.mask_bce_loss(x.transpose(2, 3).contiguous().transpose(2, 3), t)
    with pytest.raises(ValueError, match=r'mask_bce_loss.*num_frames'):
        ops.mask_bce_loss(x, t, torch.tensor([3, 2, 1], dtype=torch.int32, device=DEV))
    with pytest.raises(ValueError, match=r'mask_bce_loss.*one length'):
        ops.mask_bce_loss(x, t, [3, 4])
    with pytest.raises(ValueError, match=r'mask_bce_loss.*no gradient'):
        ops.mask_bce_loss(x, t.requires_grad_())


def _step(x, target, frames, power, reduction, gp, gw):
    from padertorch_amd import ops
    pooled, weighted = ops.mask_bce_loss(x, target, frames, power, reduction)
    grad, = torch.autograd.grad((pooled * gp).sum() + (weighted * gw).sum(), x)
    return [pooled.detach(), weighted.detach(), grad]


@pytest.mark.parametrize('reduction', ['mean', 'median'])
def test_bit_reproducible_and_capturable(reduction):
    """Two eager runs agree bit for bit; forward + backward captured ONCE at the padded shape and replayed with two length patterns
    and contents (``num_frames`` is device data) give the eager bits of each pattern."""
    from padertorch_amd.ops import capture
    B, C, T, F, _, _ = SHAPES['many']
    logits, target, powers, gp, gw = drawn('many', reduction)
    gp, gw = torch.from_numpy(gp).to(DEV), torch.from_numpy(gw).to(DEV)
    patterns = [([300, 171], 1.), ([97, 300], -0.5)]
    static = dict(x=place(logits, 'estimator').requires_grad_(), t=torch.from_numpy(target).to(DEV),
                  p=torch.from_numpy(powers['complex']).to(DEV), n=torch.zeros(B, dtype=torch.int32, device=DEV))

    def load(frames, scale):
        with torch.no_grad():
            static['x'].copy_(torch.from_numpy(logits * scale))
            static['n'].copy_(torch.tensor(frames, dtype=torch.int32))

    eager = []
    for frames, scale in patterns:
        load(frames, scale)
        eager.append([v.clone() for v in _step(static['x'], static['t'], static['n'], static['p'], reduction, gp, gw)])
        again = _step(static['x'], static['t'], static['n'], static['p'], reduction, gp, gw)
        assert all(torch.equal(a, b) for a, b in zip(eager[-1], again))
    assert not torch.equal(eager[0][0], eager[1][0])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        _step(static['x'], static['t'], static['n'], static['p'], reduction, gp, gw)         # eager warm-up on the capture stream
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with capture.capture_mode():
        with torch.cuda.graph(graph, stream=side):
            captured = _step(static['x'], static['t'], static['n'], static['p'], reduction, gp, gw)
    for (frames, scale), want in zip(patterns, eager):
        load(frames, scale)
        graph.replay()
        torch.cuda.synchronize()
        for i, (a, b) in enumerate(zip(captured, want)):
            assert torch.equal(a, b), (frames, i)


# ------------------------------------------------------------------------------------------------ the model against g19
def batch_of(g19, case, p, only=None, stft='device'):
    pick = range(len(case['frames'])) if only is None else [only]
    spectra = [g19[p + f'stft{b}'] for b in pick]
    batch = dict(observation_abs=[torch.from_numpy(np.abs(s)).to(DEV) for s in spectra],
                 num_frames=[case['frames'][b] for b in pick],
                 speech_mask_target=[torch.from_numpy(g19[p + f'speech{b}']).to(DEV) for b in pick])
    if case['noise']:
        batch['noise_mask_target'] = [torch.from_numpy(g19[p + f'noise{b}']).to(DEV) for b in pick]
    if case['stft']:
        batch['observation_stft'] = spectra if stft == 'numpy' else [torch.from_numpy(s).to(DEV) for s in spectra]
    return batch


def scalars_of(review, names):
    return np.array([float(review['scalars'][k].detach()) for k in names[:-1]] + [float(review['loss'].detach())])


@pytest.mark.parametrize('c', ['1', '2', '3min', '3max', '4'])
def test_model_matches_the_reference_fp64(g19, c):
    net, case, p = build_model(g19, c)
    net.to(DEV)
    names = json.loads(str(g19[p + 'names']))
    params = dict(net.named_parameters())
    batch = batch_of(g19, case, p)
    out = net(batch)
    for key, value in out.items():
        assert isinstance(value, list) and [tuple(v.shape)[:2] for v in value] == [(case['C'], n) for n in case['frames']]
        share(f'{c} {key}', value.padded.detach().cpu().numpy(), g19[p + 'out64_' + key], VALUE)
    review = net.review(batch, out)
    assert sorted(review) == ['loss', 'scalars']
    scalar_names = json.loads(str(g19[p + 'scalar_names']))
    assert sorted(list(review['scalars']) + ['loss']) == sorted(scalar_names)
    share(f'{c} scalars', scalars_of(review, scalar_names), g19[p + 'scalars64'], SCALAR, relative_to_max=False)
    grads = torch.autograd.grad(review['loss'], [params[n] for n in names])
    worst = max(share(f'{c} d {n}', g.cpu().numpy(), g19[p + 'g64_' + n], GRAD) for n, g in zip(names, grads))
    print(f'mask_loss ratio {c} worst gradient: {worst:.4f}')
    # the reference's own test: the loss of a minibatch is the sum of its examples' losses.  Every example alone gives the reference's
    # loss of that example alone; the sum is the minibatch's loss where the estimator treats an example in a batch as it does alone:
    # for C > 1 and B > 1 its fold '(c b) t f -> b c t f' of an example-major flattening (modul.py:131, kept: see modul.py here) hands an
    # example channels of its neighbours, and the reference's own fp64 losses do not add up either (case 1: 4.16649 against 4.16270).
    single = [float(net.review(one, net(one))['loss']) for one in (batch_of(g19, case, p, only=b) for b in range(len(case['frames'])))]
    share(f'{c} single-example losses', single, g19[p + 'single64'], SCALAR, relative_to_max=False)
    if abs(g19[p + 'single64'].sum() - g19[p + 'scalars64'][-1]) <= 0.5 * SCALAR * g19[p + 'scalars64'][-1]:      # cases 2, 3min, 3max
        share(f'{c} sum of the single-example losses', sum(single), float(review['loss']), SCALAR, relative_to_max=False)
    else:
        assert case['C'] > 1 and len(case['frames']) > 1, c
    # a caller that replaces an entry gets the entries padded instead of the storage: the same loss
    out = net(batch)
    key = 'speech_mask_logits'
    out[key][-1] = out[key][-1].clone()
    assert not out[key].intact()
    share(f'{c} loss from replaced entries', float(net.review(batch, out)['loss']), float(review['loss']), 1e-6, relative_to_max=False)
    net.create_snapshot = True
    assert sorted(net.review(batch, net(batch))) == sorted(json.loads(str(g19[p + 'review_keys'])))


def test_model_takes_the_stft_from_the_host_and_padded_targets(g19):
    net, case, p = build_model(g19, '2')
    net.to(DEV)
    scalar_names = json.loads(str(g19[p + 'scalar_names']))
    assert 'power_weighted_mask_loss' in scalar_names
    batch = batch_of(g19, case, p, stft='numpy')
    share('2 scalars, numpy stft', scalars_of(net.review(batch, net(batch)), scalar_names), g19[p + 'scalars64'], SCALAR,
          relative_to_max=False)
    for key in ('speech_mask_target', 'noise_mask_target', 'observation_stft'):          # equal lengths: the padded tensors themselves
        batch[key] = torch.stack([torch.as_tensor(v).to(DEV) for v in batch[key]])
    share('2 scalars, padded tensors', scalars_of(net.review(batch, net(batch)), scalar_names), g19[p + 'scalars64'], SCALAR,
          relative_to_max=False)


def test_one_optimizer_step(g19, tmp_path):
    import padertorch_amd as pt
    net, case, p = build_model(g19, '1')
    trainer = pt.Trainer(net, tmp_path, pt.optimizer.Adam(gradient_clipping=1.))
    trainer.to(torch.device(DEV))
    net.train()
    before = {k: v.detach().clone() for k, v in net.named_parameters()}
    loss, _, _, _ = trainer.train_step(net, batch_of(g19, case, p), DEV)
    assert loss.dim() == 0 and bool(torch.isfinite(loss))
    share('1 loss through the trainer', float(loss), g19[p + 'scalars64'][-1], SCALAR, relative_to_max=False)
    loss.backward()
    for k, v in net.named_parameters():
        assert v.grad is not None and bool(torch.isfinite(v.grad).all()) and float(v.grad.abs().max()) > 0, k
    trainer.optimizer_step()
    for k, v in net.named_parameters():
        assert not torch.equal(v.detach(), before[k]), k


def test_reconstruction_loss_and_missing_inputs(g19):
    """``speech_prediction`` (which ``MaskEstimator`` never emits) with ``speech_target``: the reference's ``F.mse_loss`` per example,
    summed; the mask losses are present only when their inputs are; the weighted sum is reported whenever the STFT is in the batch."""
    net, case, p = build_model(g19, '2')
    net.to(DEV)
    batch = batch_of(g19, case, p)
    out = dict(net(batch))
    rng = np.random.RandomState(2)
    batch['speech_target'] = [torch.from_numpy(rng.rand(*v.shape).astype(np.float32)).to(DEV) for v in out['speech_mask_logits']]
    out['speech_prediction'] = [torch.from_numpy(rng.rand(*v.shape).astype(np.float32)).to(DEV).requires_grad_()
                                for v in out['speech_mask_logits']]
    del batch['noise_mask_target']
    review = net.review(batch, out)
    assert sorted(review['scalars']) == ['power_weighted_mask_loss', 'reconstruction_loss', 'speech_mask_loss']
    want = sum(float(torch.nn.functional.mse_loss(t.double(), e.detach().double()))
               for t, e in zip(batch['speech_target'], out['speech_prediction']))
    share('reconstruction loss', float(review['scalars']['reconstruction_loss'].detach()), want, VALUE, relative_to_max=False)
    share('loss with the reconstruction loss', float(review['loss'].detach()),
          want + float(review['scalars']['speech_mask_loss'].detach()), VALUE, relative_to_max=False)
    grads = torch.autograd.grad(review['loss'], out['speech_prediction'])
    e, t = out['speech_prediction'][0].detach().double(), batch['speech_target'][0].double()
    share('d speech_prediction', grads[0].cpu().numpy(), (2 * (e - t) / e.numel()).cpu().numpy(), GRAD)
