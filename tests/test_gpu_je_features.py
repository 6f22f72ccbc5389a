"""The feature kernels (csrc/je_features.hip) against the float64 restatement tests/je_features_ref.py on explicit draws, and
NormalizedLogMelExtractor against the reference's own float64 run (tests/golden/g29_je_features.npz, make_golden_je_features.py).

Gates are on max |got - float64|.  The static log-mel keeps the project's mel gate (rtol = atol = 1e-5, test_gpu_logmel.py); every other
gate is four times the largest error of the restatement's float32 run (``dt=np.float32``) on the very cases below, measured on the CPU;
the module gates are the generator's (four times the reference's float32 run).  Masked values, edge deltas and the values on all-zero
frames are compared with equality."""
import importlib.util
import itertools
from pathlib import Path

import numpy as np
import pytest
import torch

import je_features_ref as ref

pytestmark = pytest.mark.gpu
GOLDEN = Path(__file__).resolve().parent / 'golden'
B, C, M, STFT, RATE = 3, 2, 10, 64, 16000
F = STFT // 2 + 1
MEL_GATE = 1e-5          # rtol = atol, the existing gate of the static filterbank
WARPED_GATE = 1.7e-6     # warped log-mel: float32 restatement off by 4.24e-7 (worst of the 4 cases)
IPD_GATE = 2.2e-6        # cos / sin: float32 restatement off by 5.41e-7
SHAPE_GATE = 6.8e-6      # warp + blur + deltas: float32 restatement off by 1.69e-6 (worst of the 20 cases)
TAIL_GATE = 4.9e-6       # normalise .. masks: float32 restatement off by 1.22e-6 (worst of the 18 cases)


def _dev(a, dtype=torch.float32):
    return None if a is None else torch.as_tensor(np.asarray(a), dtype=dtype).cuda()


def _close(got, want, gate, what):
    err = float(np.abs(got.double().cpu().numpy() - want).max())
    print(f'{what}: max error {err:.3g} (gate {gate:.3g})')
    assert err <= gate, (what, err, gate)


def front_case(warped, partner, ipd, tile):
    """Arguments of one kernel A case; row 2's last five frames are all zero (and stay so: its lambda is 0)."""
    from padertorch_amd.contrib.je.modules.features import MelTransform, _hz2mel, _mel2hz
    rng = np.random.RandomState(29)
    x = rng.randn(B, C, tile + 3, F, 2).astype(np.float32)
    x[2, :, -5:] = 0.
    mel = MelTransform(RATE, STFT, M)
    kw, edges = dict(max_bin=mel.fbanks.argmax(0).numpy(), pairs=((0, 1),) if ipd else ()), None
    if warped:          # piecewise linear on the mel scale: the lower 60 % stretched by alpha, the rest squeezed; row 0 unwarped
        e = np.linspace(_hz2mel(50., True), _hz2mel(RATE / 2, True), M + 2)
        knee, alpha = e[0] + .6 * (e[-1] - e[0]), np.array([1., 1.15, .85])[:, None]
        low = e[0] + alpha * (e - e[0])
        high = e[-1] - (e[-1] - e) * (e[-1] - (e[0] + alpha * (knee - e[0]))) / (e[-1] - knee)
        edges = _mel2hz(np.where(e <= knee, low, high), True).astype(np.float32)
        kw.update(edges_hz=edges, bin_hz=RATE / STFT)
    if partner:
        kw.update(gain=np.array([.5, 1.5, 2.]), partner=np.array([1, 2, 0]), partner_gain=np.array([1.2, .7, .9]), lam=np.array([1., 1., 0.]))
    fb = ref.triangles(edges, F, RATE / STFT) if warped else mel.fbanks.numpy().T[None].astype(np.float64)
    return x, mel, kw, fb


@pytest.mark.parametrize('warped,partner,ipd', list(itertools.product((False, True), repeat=3)))
def test_logmel_front(warped, partner, ipd):
    from padertorch_amd.ops import je_features as ops
    x, mel, kw, fb = front_case(warped, partner, ipd, ops.front_tile())
    want, want_cos, want_sin = ref.front(x, fb, **{k: v for k, v in kw.items() if k not in ('edges_hz', 'bin_hz')})
    got, cos, sin = ops.logmel_front(_dev(x), mel._bands, **kw)
    assert got.shape == want.shape
    if warped:
        _close(got, want, WARPED_GATE, 'warped log-mel')
    else:
        np.testing.assert_allclose(got.cpu().numpy(), want, rtol=MEL_GATE, atol=MEL_GATE)
    assert (got[2, :, :, -5:].cpu().numpy() == np.float32(np.log(np.float64(np.float32(1e-12))))).all()
    if ipd:
        _close(cos, want_cos, IPD_GATE, 'ipd cos')
        _close(sin, want_sin, IPD_GATE, 'ipd sin')
        assert (cos[2, :, :, -5:] == 1).all() and (sin[2, :, :, -5:] == 0).all()


SHAPE_CASES = [(w, k, d, M) for w in (False, True) for k in (0, 3, 5) for d in (0, 1, 2)] + [(False, 3, 2, 2), (True, 5, 2, 3)]


def shape_case(warp, k, d, m, tile):
    """``T' = tile + 3``; with a warp the input is 7 frames shorter and row 0 hits integers only, all rows saturate at ``T - 1``."""
    from padertorch_amd.contrib.je.modules.augment import gaussian
    from padertorch_amd.contrib.je.modules.features import DeltaExtractor
    rng = np.random.RandomState(30)
    To = tile + 3
    T = To - 7 if warp else To
    kw = dict(seq_len=[To, To - 5, 3])
    if warp:
        kw['tau'] = np.minimum(np.arange(To)[None] / np.array([1., 1.3, 1 / 1.1])[:, None], T - 1)
    if k:
        kw['taps'] = gaussian(k, torch.tensor([.4, 1., 2.5])).numpy()
    if d:
        kw['kd'] = DeltaExtractor(order=1).kernel.numpy()
    if d > 1:
        kw['kdd'] = DeltaExtractor(order=2).kernel.numpy()
    return (rng.randn(B, C, m, T) * 2 - 3).astype(np.float32), kw


@pytest.mark.parametrize('warp,k,d,m', SHAPE_CASES)
def test_feature_shape(warp, k, d, m):
    from padertorch_amd.ops import je_features as ops
    x, kw = shape_case(warp, k, d, m, ops.shape_tile())
    want = ref.shape(x, **kw)
    got = ops.feature_shape(_dev(x), time_indices=kw.get('tau'), taps=kw.get('taps'), delta_kernel=kw.get('kd'),
                            delta_delta_kernel=kw.get('kdd'), seq_len=kw['seq_len'])
    assert got.shape == want.shape
    _close(got, want, SHAPE_GATE, 'feature_shape')
    t, n = np.arange(want.shape[-1]), np.asarray(kw['seq_len']).reshape(B, 1, 1, 1)
    zero = np.broadcast_to((t < 2) | (t >= len(t) - 2) | (t >= n - 2), want.shape).copy()
    zero[:, :C] = False                                              # the deltas' edge frames and their frames from seq_len - 2 on
    assert (want[zero] == 0).all() and (got.cpu().numpy()[zero] == 0).all()


TAIL_STAGES = ('norm_bt', 'norm_bft', 'clamp', 'ipd', 'mixup', 'noise', 'time_masks', 'freq_masks', 'all')


def tail_case(stage, T):
    rng = np.random.RandomState(31)
    x, lens, kw = (rng.randn(B, C, M, T) * 3).astype(np.float32), [T, T - 5, 3], {}
    on = lambda *names: stage in names + ('all',)                    # noqa: E731
    if on('norm_bt', 'norm_bft'):
        shape = (1, C, 1, 1) if stage == 'norm_bft' else (1, C, M, 1)
        kw.update(mean=rng.randn(*shape).astype(np.float32), rstd=(.5 + rng.rand(*shape)).astype(np.float32), seq_len=lens)
    if on('clamp'):
        kw['clamp'] = 2.5
    if on('ipd'):
        kw.update(cos=rng.randn(B, 1, M, T).astype(np.float32), sin=rng.randn(B, 1, M, T).astype(np.float32))
    if on('mixup'):
        kw.update(partner=np.array([2, 0, 1]), lam=np.array([1., 0., .3], np.float32))
    if on('noise'):
        kw.update(noise_scale=np.array([.1, 0., .4], np.float32), noise=rng.randn(B, C + 2 * ('cos' in kw), M, T).astype(np.float32))
    if on('time_masks'):         # width 0 (row 0), up to the end of row 1's length, and a second mask
        kw['time_masks'] = (np.array([[4, T - 12, 0], [0, 2, 1]], np.int32), np.array([[4, T - 5, 2], [3, 9, 1]], np.int32))
    if on('freq_masks'):         # band 0 (row 0)
        kw['freq_masks'] = (np.array([[0, 3, M - 2]], np.int32), np.array([[2, 3, M]], np.int32))
    return x, kw


@pytest.mark.parametrize('stage,T', list(itertools.product(TAIL_STAGES, (35, 36))))       # M T % 4 != 0 and == 0: both access widths
def test_feature_tail(stage, T):
    from padertorch_amd.ops import je_features as ops
    x, kw = tail_case(stage, T)
    want = ref.tail(x, **kw)
    dev = {k: _dev(v) if k in ('mean', 'rstd', 'cos', 'sin', 'noise') else v for k, v in kw.items()}
    got = ops.feature_tail(_dev(x), ipd_cos=dev.pop('cos', None), ipd_sin=dev.pop('sin', None), **dev)
    assert got.shape == want.shape
    _close(got, want, TAIL_GATE, stage)
    if 'clamp' in kw and 'noise' not in kw and 'cos' not in kw:
        assert float(got.abs().max()) <= 2.5 < float(np.abs(x).max())
    assert (got.cpu().numpy()[want == 0] == 0).all()                 # masked elements are exactly 0


@pytest.fixture(scope='module')
def golden():
    spec = importlib.util.spec_from_file_location('make_golden_je_features', GOLDEN / 'make_golden_je_features.py')
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    return gen, dict(np.load(GOLDEN / 'g29_je_features.npz'))


@pytest.mark.parametrize('case', ['c0', 'c1', 'c2', 'c3'])
def test_extractor_against_the_reference(case, golden):
    gen, g29 = golden
    from padertorch_amd.contrib.je.modules.features import NormalizedLogMelExtractor
    if case == 'c3':             # the streams of the installed numpy / torch still give the tables the golden run drew: else "stream order"
        host, cpu = gen.draws()
        assert np.array_equal(host, g29['c3_draws_np']), 'stream order (numpy)'
        assert np.array_equal(cpu, g29['c3_draws_torch']), 'stream order (torch)'
    got = gen.run(NormalizedLogMelExtractor, case, torch.float32, 'cuda')
    for key, have in got.items():
        want = g29[key]
        assert have.shape == want.shape, key
        if key.endswith('_y'):
            err = float(np.abs(have - want).max())
            print(f'{key}: max error {err:.3g} (gate {gen.GATES[case]:.3g})')
            assert err <= gen.GATES[case], (key, err)
            assert (have[want == 0] == 0).all(), key
        else:
            np.testing.assert_allclose(have, want, rtol=1e-5, atol=1e-6, err_msg=key)       # lengths, targets, the norm's buffers


def test_refusals():
    from padertorch_amd.contrib.je.modules import augment
    from padertorch_amd.contrib.je.modules.features import DeltaExtractor, MelTransform, NormalizedLogMelExtractor
    from padertorch_amd.ops import je_features as ops
    x = torch.zeros(2, 1, 12, 6, device='cuda')
    for match, call in (
            ('F <= 1025', lambda: ops.logmel_front(torch.zeros(1, 1, 2, 2049, 2, device='cuda'), MelTransform(RATE, 4096, 40)._bands)),
            ('C <= 8', lambda: ops.logmel_front(torch.zeros(1, 9, 2, F, 2, device='cuda'), MelTransform(RATE, STFT, M)._bands)),
            ('number_of_filters <= 256', lambda: NormalizedLogMelExtractor(RATE, 1024, 257)),
            ('k <= 9', lambda: augment.GaussianBlur2d(11, lambda n: np.ones(n)).train()(x)),
            (r'\(k \+ 1\) / 2 = 5', lambda: augment.GaussianBlur2d(9, lambda n: np.ones(n)).train()(x[:, :, :4])),
            ('width 5', lambda: DeltaExtractor(width=7)(x)),
            ('B >= 2', lambda: augment.Superpose(p=1.).train()(x[:1], None))):
        with pytest.raises(NotImplementedError, match=match):
            call()
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        NormalizedLogMelExtractor(RATE, STFT, M)(torch.zeros(2, 1, 5, F, 2))
