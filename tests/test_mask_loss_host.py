"""The mask estimator's loss (``ops.mask_bce_loss``, ``csrc/mask_loss.hip``) and ``MaskEstimatorModel`` without a GPU: a numpy fp64
restatement of the op - which tests/test_gpu_mask_loss.py compares the kernels with - checked against torch on the CPU, and the
interface of the model and the op."""
import json
from pathlib import Path

import numpy as np
import pytest
import torch

GOLDEN = Path(__file__).resolve().parent / 'golden'
REDUCTIONS = ('mean', 'median', 'min', 'max')


# ------------------------------------------------------------------------------------------------ the restatement (numpy, fp64)
def ref_element_loss(x, t):
    """``max(x, 0) - x t + log1p(exp(-|x|))``."""
    x, t = np.asarray(x, np.float64), np.asarray(t, np.float64)
    return np.maximum(x, 0) - x * t + np.log1p(np.exp(-np.abs(x)))


def ref_rank(n, reduction):
    """The ascending rank the pooling selects: torch's LOWER median."""
    return dict(median=(n - 1) // 2, min=0, max=n - 1)[reduction]


def ref_weights(power):
    power = np.asarray(power)
    if np.iscomplexobj(power):
        power = power.astype(np.complex128)
        return power.real ** 2 + power.imag ** 2
    return power.astype(np.float64)


def ref_mask_bce(logits, target, frames, power=None, reduction='mean', g_pooled=None, g_weighted=None):
    """``logits, target [B, C, T, F]``, ``frames`` host ints -> ``(pooled [B], weighted [B] or None, d logits [B, C, T, F])``: the
    gradient of ``sum_b g_pooled[b] pooled[b] + g_weighted[b] weighted[b]`` with the even split among ties, zeros behind the lengths."""
    B = logits.shape[0]
    pooled, weighted = np.empty(B), (None if power is None else np.empty(B))
    grad = np.zeros(logits.shape)
    g_pooled = np.zeros(B) if g_pooled is None else np.asarray(g_pooled, np.float64)
    g_weighted = np.zeros(B) if g_weighted is None else np.asarray(g_weighted, np.float64)
    with np.errstate(all='ignore'):
        for b, n in enumerate(frames):
            x, t = logits[b, :, :n].astype(np.float64), target[b, :, :n].astype(np.float64)
            loss = ref_element_loss(x, t)
            dl = 1 / (1 + np.exp(-x)) - t
            if reduction == 'mean':
                pooled[b] = loss.mean() if loss.size else np.nan
                coef = np.full(loss.shape, 1 / max(loss.size, 1))
            elif loss.size == 0 or np.isnan(loss).any():
                pooled[b], coef = np.nan, np.zeros(loss.shape)
            else:
                pooled[b] = np.sort(loss, axis=None)[ref_rank(loss.size, reduction)]
                chosen = loss == pooled[b]
                coef = chosen / chosen.sum()
            grad[b, :, :n] = g_pooled[b] * coef * dl
            if power is not None:
                w = ref_weights(power[b, :, :n])
                weighted[b] = (loss * w).sum() / w.sum()
                grad[b, :, :n] += g_weighted[b] * w / w.sum() * dl
    return pooled, weighted, grad


def ref_gap(logits, target, frames, reduction):
    """Smallest relative distance of a selected loss from its nearest unequal neighbour (inf for the mean): below ~1e-5 fp32 rounding
    may select another element than fp64 does."""
    if reduction == 'mean':
        return np.inf
    gap = np.inf
    for b, n in enumerate(frames):
        loss = np.sort(ref_element_loss(logits[b, :, :n], target[b, :, :n]), axis=None)
        if loss.size == 0:
            continue
        v = loss[ref_rank(loss.size, reduction)]
        others = loss[loss != v]
        if others.size:
            gap = min(gap, float(np.abs(others - v).min() / abs(v)))
    return gap


def tie_case(rng, n):
    """``n`` (logit, target) pairs in random order whose minimum, maximum and (lower) median loss are each attained exactly 3 times:
    ``(x [n], t [n], {reduction: positions})``."""
    m = n - 6
    assert m >= 3
    x, t = rng.randn(m) * 2, rng.uniform(0, 1, m)
    order = np.argsort(ref_element_loss(x.astype(np.float32), t.astype(np.float32)))
    picks = dict(min=order[0], max=order[-1], median=order[(m - 1) // 2])
    src = np.concatenate([np.arange(m)] + [np.repeat(i, 2) for i in picks.values()])
    perm = rng.permutation(n)
    src = src[perm]
    x, t = x[src].astype(np.float32), t[src].astype(np.float32)
    return x, t, {k: np.flatnonzero(src == i) for k, i in picks.items()}


# ------------------------------------------------------------------------------------------------ shared with the GPU tests
def load_g19():
    d = dict(np.load(GOLDEN / 'g19_mask_model.npz', allow_pickle=False))
    d['cases'] = json.loads(str(d['cases']))
    return d


@pytest.fixture(scope='module')
def g19():
    return load_g19()


def build_model(g19, c, **kwargs):
    """``MaskEstimatorModel`` around the tiny estimator of tests/test_mask_estimator.py with case ``c``'s parameters."""
    from padertorch_amd.contrib.jensheit.mask_estimator_example import MaskEstimatorModel
    case = g19['cases'][c]
    net = MaskEstimatorModel.from_defaults(num_features=case['F'], reduction=kwargs.pop('reduction', case['reduction']),
                                           recurrent=dict(hidden_size=8),
                                           fully_connected=dict(hidden_size=[16, 12, 16], dropout=0., input_size=16), **kwargs)
    p = c + '_'
    net.load_state_dict({k: torch.from_numpy(g19[p + 'p_' + k]) for k in json.loads(str(g19[p + 'keys']))}, strict=True)
    return net, case, p


# ------------------------------------------------------------------------------------------------ the restatement against torch
def _torch_reference(logits, target, frames, power, reduction, g_pooled, g_weighted):
    pool = dict(mean=torch.mean, median=torch.median, min=torch.min, max=torch.max)[reduction]
    x = torch.tensor(logits, dtype=torch.float64, requires_grad=True)
    t = torch.tensor(target, dtype=torch.float64)
    pooled, weighted, total = [], [], 0.
    for b, n in enumerate(frames):
        loss = torch.nn.functional.binary_cross_entropy_with_logits(x[b, :, :n], t[b, :, :n], reduction='none')
        pooled.append(pool(loss))
        total = total + g_pooled[b] * pooled[-1]
        if power is not None:
            w = torch.tensor(ref_weights(power[b, :, :n]))
            weighted.append(torch.sum(loss * w) / torch.sum(w))
            total = total + g_weighted[b] * weighted[-1]
    total.backward()
    return (torch.stack(pooled).detach().numpy(), torch.stack(weighted).detach().numpy() if weighted else None, x.grad.numpy())


@pytest.mark.parametrize('reduction', REDUCTIONS)
@pytest.mark.parametrize('power', ['none', 'real', 'complex'])
def test_restatement_against_torch(reduction, power):
    rng = np.random.RandomState(19)
    B, C, T, F, frames = 3, 2, 7, 5, [7, 4, 1]
    logits, target = rng.randn(B, C, T, F) * 2, rng.uniform(-0.5, 1.5, (B, C, T, F))
    pw = dict(none=None, real=rng.uniform(0, 2, (B, C, T, F)), complex=rng.randn(B, C, T, F) + 1j * rng.randn(B, C, T, F))[power]
    gp, gw = rng.randn(B), rng.randn(B)
    got = ref_mask_bce(logits, target, frames, pw, reduction, gp, gw)
    want = _torch_reference(logits, target, frames, pw, reduction, gp, gw)
    np.testing.assert_allclose(got[0], want[0], rtol=1e-12)
    if pw is None:
        assert got[1] is None
    else:
        np.testing.assert_allclose(got[1], want[1], rtol=1e-12)
    np.testing.assert_allclose(got[2], want[2], rtol=1e-10, atol=1e-14)
    for b, n in enumerate(frames):
        assert not got[2][b, :, n:].any()


@pytest.mark.parametrize('reduction', ['median', 'min', 'max'])
@pytest.mark.parametrize('n', [15, 16])
def test_restatement_splits_ties_like_torch(reduction, n):
    """Deliberate ties: the extreme and the median are each attained 3 times; torch splits the gradient evenly, and so does the
    restatement."""
    x, t, where = tie_case(np.random.RandomState(n), n)
    logits, target = x.reshape(1, 1, 1, n), t.reshape(1, 1, 1, n)
    got = ref_mask_bce(logits, target, [1], None, reduction, [1.5])
    want = _torch_reference(logits, target, [1], None, reduction, [1.5], None)
    np.testing.assert_allclose(got[0], want[0], rtol=1e-14)
    np.testing.assert_allclose(got[2], want[2], rtol=1e-12, atol=1e-15)
    assert np.flatnonzero(got[2]).tolist() == sorted(where[reduction].tolist()) and len(where[reduction]) == 3
    assert ref_rank(4, 'median') == 1 and ref_rank(5, 'median') == 2        # the lower median


# ------------------------------------------------------------------------------------------------ interface
def test_keys_reduction_names_and_config(g19):
    from padertorch_amd.contrib.jensheit.mask_estimator_example import MaskEstimator, MaskEstimatorModel, MaskLossKeys
    assert {k: v for k, v in vars(MaskLossKeys).items() if not k.startswith('_')} == dict(
        NOISE_MASK='noise_mask_loss', SPEECH_MASK='speech_mask_loss', WEIGHTED_NOISE_MASK='power_weighted_noise_mask_loss',
        WEIGHTED_SPEECH_MASK='power_weighted_speech_mask_loss', MASK='mask_loss', WEIGHTED_MASK='power_weighted_mask_loss',
        TOTAL_MASK='total_mask_loss', VAD='VAD_loss', REC='reconstruction_loss')
    config = {}
    MaskEstimatorModel.finalize_dogmatic_config(config)
    assert config == dict(estimator=dict(factory=MaskEstimator))
    estimator = MaskEstimator.from_defaults(num_features=5, recurrent=dict(hidden_size=8),
                                            fully_connected=dict(hidden_size=[16], input_size=16))
    default = MaskEstimatorModel(estimator)
    assert default.reduction == 'average' and default.pooling == 'mean' and default.sample_rate == 16000 and default.transformer is None
    assert MaskEstimatorModel(estimator, reduction='median').pooling == 'median'
    with pytest.raises(ValueError, match='sum'):
        MaskEstimatorModel(estimator, reduction='sum')
    for c in g19['cases']:
        net, _, p = build_model(g19, c)
        assert list(net.state_dict()) == json.loads(str(g19[p + 'keys']))
        assert all(k.startswith('estimator.') for k in net.state_dict())
        assert [n for n, _ in net.named_parameters()] == json.loads(str(g19[p + 'names']))


def test_op_argument_errors():
    from padertorch_amd import ops
    from padertorch_amd.ops import losses
    assert ops.mask_bce_loss is losses.mask_bce_loss
    x, t = torch.zeros(2, 1, 3, 4), torch.zeros(2, 1, 3, 4)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        ops.mask_bce_loss(x, t)
    with pytest.raises(NotImplementedError):
        torch.ops.ptmi.mask_loss_forward(x, t, None, None, 0)           # CUDA key only
    with pytest.raises(ValueError, match=r'mask_bce_loss.*reduction'):
        ops.mask_bce_loss(x, t, reduction='sum')
    with pytest.raises(ValueError, match=r'mask_bce_loss.*\(2, 1, 3, 4\).*\(2, 1, 3, 5\)'):
        ops.mask_bce_loss(x, torch.zeros(2, 1, 3, 5))
    with pytest.raises(ValueError, match=r'mask_bce_loss.*\(2, 3, 4\)'):
        ops.mask_bce_loss(x[:, 0], t[:, 0])
    with pytest.raises(ValueError, match=r'mask_bce_loss.*float64'):
        ops.mask_bce_loss(x.double(), t)
    with pytest.raises(ValueError, match=r'mask_bce_loss.*power.*\(2, 1, 3, 3\)'):
        ops.mask_bce_loss(x, t, power=torch.zeros(2, 1, 3, 3))
    with pytest.raises(ValueError, match=r'mask_bce_loss.*power.*int32'):
        ops.mask_bce_loss(x, t, power=torch.zeros(2, 1, 3, 4, dtype=torch.int32))


def test_vad_is_refused_and_channels_are_removed(g19):
    from padertorch_amd.contrib.jensheit.mask_estimator_example.model import maybe_remove_channel
    net, _, _ = build_model(g19, '1')
    with pytest.raises(NotImplementedError, match='VAD'):
        net.review(dict(vad=[torch.zeros(1, 2, 1)]), dict(vad_logits=[torch.zeros(1, 2, 1)]))
    signal = np.arange(6.).reshape(2, 3)
    assert maybe_remove_channel(signal).tolist() == [0., 1., 2.]
    assert maybe_remove_channel(torch.from_numpy(signal), ref_channel=1).tolist() == [3., 4., 5.]
    assert maybe_remove_channel(signal[0]) is not None and maybe_remove_channel(signal, exp_dim=2) is signal
    with pytest.raises(ValueError):
        maybe_remove_channel(signal[None, None])
    with pytest.raises(ValueError):
        maybe_remove_channel([1., 2.])
    with pytest.raises(AssertionError):
        maybe_remove_channel(np.zeros((20, 3)))


def test_mask_list_is_a_plain_list():
    from padertorch_amd.contrib.jensheit.mask_estimator_example.model import MaskList
    padded = torch.arange(2 * 3 * 4 * 5.).reshape(2, 3, 4, 5)[..., :2]               # a strided view, as the estimator's halves
    entries = MaskList(padded, [4, 2], lengths_dev=torch.tensor([4, 2], dtype=torch.int32))
    assert isinstance(entries, list) and [tuple(e.shape) for e in entries] == [(3, 4, 2), (3, 2, 2)] and entries.intact()
    assert torch.equal(entries[1], padded[1, :, :2])
    entries[1] = entries[1].clone()
    assert not entries.intact()
    swapped = MaskList(padded, [4, 2], lengths_dev=entries.lengths_dev)
    swapped.reverse()
    assert not swapped.intact()
