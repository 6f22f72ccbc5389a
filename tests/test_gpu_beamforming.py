"""Mask-based MVDR beamforming on the GPU (``csrc/beamform.hip`` through ``ops.beamforming``) against the fp64 numpy restatement of
``tests/test_beamforming_host.py`` on the same fp32 inputs.

Error measure: max abs deviation over the max abs value of the fp64 result, over EVERY element.  Tolerance, per case and quantity:
8 times the deviation of the same restatement run in complex64 / float32 from its fp64 run (never anything the kernels produce); the
kernels sum in fp64, the factor covers another order of summation.  A case is computed once (restatement and kernels) and shared by
the tests that look at it.

Case: ``Y = a_f s(t, f) + 0.5 n_c(t, f)`` with half of the ``s`` entries zero, speech mask ``0.8 [s != 0] + 0.2 U`` per channel, noise
mask ``1 - speech``.
"""
import functools

import numpy as np
import pytest
import torch

from test_beamforming_host import ref_apply, ref_median, ref_psd, ref_souden

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1, 9, 5), (2, 2, 9, 65), (2, 3, 33, 65), (3, 6, 70, 129), (1, 8, 130, 67), (1, 6, 600, 513)]
FRAMES = {(3, 6, 70, 129): [70, 41, 7]}
FACTOR = 8


def cnormal(rng, *shape):
    return (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)) / np.sqrt(2)


def make_inputs(shape, seed=0):
    B, C, T, F = shape
    rng = np.random.default_rng(seed)
    a = cnormal(rng, B, C, 1, F)
    s = cnormal(rng, B, 1, T, F) * (rng.uniform(size=(B, 1, T, F)) < 0.5)
    Y = (a * s + 0.5 * cnormal(rng, B, C, T, F)).astype(np.complex64)
    speech = (0.8 * (s != 0) + 0.2 * rng.uniform(size=(B, C, T, F))).astype(np.float32)
    return Y, speech, (1 - speech).astype(np.float32)


def deviation(got, want):
    return float(np.abs(np.asarray(got) - want).max() / np.abs(want).max())


def chain(Y, ms, mn, frames, ref):
    """The restatement in the precision of its inputs: every quantity the tests compare."""
    out = dict(psd_s=ref_psd(Y, ms, frames), psd_n=ref_psd(Y, mn, frames), psd_s_raw=ref_psd(Y, ms, frames, normalize=False),
               psd_n_raw=ref_psd(Y, mn, frames, normalize=False), cov=ref_psd(Y, None, frames))
    out['w'] = ref_souden(out['psd_s'], out['psd_n'], ref)[0]
    out['Z'] = ref_apply(out['w'], Y, frames)
    return out


def dev_tensor(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def host(x):
    return x.cpu().numpy()


def run_kernels(Y, speech, noise, frames, ref):
    from padertorch_amd import ops
    fr = None if frames is None else torch.tensor(frames, dtype=torch.int32).cuda()
    Yd, sd, nd = dev_tensor(Y), dev_tensor(speech), dev_tensor(noise)
    got = dict(psd_s=ops.get_power_spectral_density_matrix(Yd, sd, frames=fr), psd_n=ops.get_power_spectral_density_matrix(Yd, nd, frames=fr),
               psd_s_raw=ops.get_power_spectral_density_matrix(Yd, sd, frames=fr, normalize=False),
               psd_n_raw=ops.get_power_spectral_density_matrix(Yd, nd, frames=fr, normalize=False),
               cov=ops.get_power_spectral_density_matrix(Yd, frames=fr))
    got['w'] = ops.get_mvdr_vector_souden(got['psd_s'], got['psd_n'], ref)
    got['Z'] = ops.apply_beamforming_vector(got['w'], Yd, frames=fr)
    got['Z_fused'] = ops.mask_beamforming(Yd, sd, nd, frames=fr, ref_channel=ref)
    return got, (Yd, sd, nd, fr)


@functools.lru_cache(maxsize=None)
def case(shape):
    """Inputs, the fp64 restatement, the tolerances from its float32 run and the kernels' results: once per shape."""
    Y, speech, noise = make_inputs(shape)
    frames, ref = FRAMES.get(shape), shape[1] // 2
    ms, mn = ref_median(speech), ref_median(noise)                      # float32, exactly what the kernel takes
    want = chain(Y.astype(np.complex128), ms.astype(np.float64), mn.astype(np.float64), frames, ref)
    single = chain(Y, ms, mn, frames, ref)
    assert all(v.dtype in (np.complex64, np.float32) for v in single.values())
    tol = {k: FACTOR * deviation(single[k], want[k]) for k in want}
    got, device = run_kernels(Y, speech, noise, frames, ref)
    return dict(inputs=(Y, speech, noise), reduced=(ms, mn), frames=frames, ref=ref, want=want, tol=tol, got=got, device=device)


@pytest.mark.parametrize('shape', SHAPES, ids=str)
def test_psd_vector_and_output_against_the_restatement(shape):
    c = case(shape)
    errors = {k: deviation(host(c['got'][k]), c['want'][k]) for k in c['want']}
    errors['Z_fused'] = deviation(host(c['got']['Z_fused']), c['want']['Z'])
    cond = np.linalg.cond(c['want']['psd_n']).max()
    print(f'\n{shape} cond(Phi_n) <= {cond:.1f}: ' + ', '.join(f'{k} {errors[k]:.2e} (tol {c["tol"][k.replace("_fused", "")]:.2e})' for k in errors))
    for k, e in errors.items():
        assert e <= c['tol'][k.replace('_fused', '')], (k, e, c['tol'][k.replace('_fused', '')])
    assert c['got']['psd_s'].dtype == torch.complex128 and c['got']['w'].dtype == c['got']['Z'].dtype == torch.complex64
    assert torch.equal(c['got']['Z'], c['got']['Z_fused'])            # one launch for both PSD matrices gives the same bits


@pytest.mark.parametrize('shape', SHAPES, ids=str)
def test_psd_is_exactly_hermitian_and_runs_are_bit_identical(shape):
    from padertorch_amd import ops
    c = case(shape)
    for k in ('psd_s', 'psd_n', 'psd_s_raw', 'cov'):
        P = c['got'][k]
        assert torch.equal(P, P.transpose(-1, -2).conj().resolve_conj()), k
        assert float(torch.diagonal(P, dim1=-2, dim2=-1).imag.abs().max()) == 0.
    Yd, sd, nd, fr = c['device']
    again = ops.mask_beamforming(Yd, sd, nd, frames=fr, ref_channel=c['ref'])
    assert torch.equal(again, c['got']['Z'])
    assert torch.equal(ops.get_power_spectral_density_matrix(Yd, nd, frames=fr), c['got']['psd_n'])


@pytest.mark.parametrize('shape', SHAPES, ids=str)
def test_median_path_equals_a_reduced_mask_bit_for_bit(shape):
    from padertorch_amd import ops
    c = case(shape)
    Yd, _, _, fr = c['device']
    for k, m in zip(('psd_s', 'psd_n'), c['reduced']):
        reduced = ops.get_power_spectral_density_matrix(Yd, dev_tensor(m), frames=fr, channel_reduce=None)
        assert torch.equal(reduced, c['got'][k]), k


def test_frames_zero_the_tail_and_hide_what_lies_behind_them():
    from padertorch_amd import ops
    shape = (3, 6, 70, 129)
    c = case(shape)
    Y, speech, noise = (x.copy() for x in c['inputs'])
    Z = c['got']['Z']
    for b, n in enumerate(c['frames']):
        assert not bool(Z[b, n:].abs().any()) and bool(Z[b, :n].abs().all())
        Y[b, :, n:] = 1e30 * (1 + 1j)                                     # whatever lies behind the valid frames ...
        speech[b, :, n:] = np.nan
        noise[b, :, n:] = -7.
    _, _, _, fr = c['device']
    changed = ops.mask_beamforming(dev_tensor(Y), dev_tensor(speech), dev_tensor(noise), frames=fr, ref_channel=c['ref'])
    assert torch.equal(changed, Z)                                        # ... changes nothing, bit for bit
    assert torch.equal(ops.get_power_spectral_density_matrix(dev_tensor(Y), frames=fr), c['got']['cov'])


def test_three_dimensional_inputs_are_a_batch_of_one():
    from padertorch_amd import ops
    c = case((1, 8, 130, 67))
    Yd, sd, nd, _ = c['device']
    assert torch.equal(ops.mask_beamforming(Yd[0], sd[0], nd[0], ref_channel=c['ref']), c['got']['Z'][0])
    psd = ops.get_power_spectral_density_matrix(Yd[0], sd[0])
    assert psd.shape == (67, 8, 8) and torch.equal(psd, c['got']['psd_s'][0])
    w, ref = ops.get_mvdr_vector_souden(psd, c['got']['psd_n'][0], c['ref'], return_ref_channel=True)
    assert torch.equal(w, c['got']['w'][0]) and ref.dtype == torch.int32 and ref.tolist() == [c['ref']]


# ---- automatic reference channel --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('C,seed', [(2, 0), (3, 0), (6, 2), (8, 0)])
def test_reference_channel_is_chosen_on_the_device(C, seed):
    """``Phi = A A^H / 2C`` with ``A [F = 17, C, 2C]`` complex normal, row ``c`` of the target's ``A`` scaled by ``linspace(1, 2, C)[c]``
    (the second example of the batch, drawn after the first: by ``linspace(3, 1, C)[c]``)."""
    from padertorch_amd import ops
    rng = np.random.default_rng(seed)
    F = 17

    def draw():
        return rng.standard_normal((F, C, 2 * C)) + 1j * rng.standard_normal((F, C, 2 * C))
    scale = np.linspace(1, 2, C)[None, :, None]
    A = [[draw() * scale, draw()], [draw() * (2 * scale[:, ::-1] - 1), draw()]]                                # per example: target, noise
    Ps, Pn = (np.stack([np.einsum('fck,fdk->fcd', X[i], X[i].conj()) / (2 * C) for X in A]) for i in range(2))
    w64, ref64, ratio = ref_souden(Ps, Pn)
    top = np.sort(ratio, axis=1)
    gap = (top[:, -1] - top[:, -2]) / top[:, -1]
    print(f'\nC={C} seed={seed}: chosen {ref64.tolist()}, gap between the two best ratios {np.round(100 * gap, 1).tolist()} %')
    assert (gap >= 0.01).all(), gap
    _, ref32, _ = ref_souden(Ps.astype(np.complex64), Pn.astype(np.complex64))
    assert ref32.tolist() == ref64.tolist()
    tol = FACTOR * deviation(ref_souden(Ps.astype(np.complex64), Pn.astype(np.complex64))[0], w64)
    w, ref = ops.get_mvdr_vector_souden(dev_tensor(Ps), dev_tensor(Pn), return_ref_channel=True)
    assert ref.dtype == torch.int32 and ref.is_cuda and ref.tolist() == ref64.tolist()
    err = deviation(host(w), w64)
    print(f'w {err:.2e} (tol {tol:.2e})')
    assert err <= tol
    for r in range(C):                                                    # an int means that column, for every example
        assert deviation(host(ops.get_mvdr_vector_souden(dev_tensor(Ps), dev_tensor(Pn), r)), ref_souden(Ps, Pn, r)[0]) <= tol
    one, ref_one = ops.get_mvdr_vector_souden(dev_tensor(Ps[1]), dev_tensor(Pn[1]), return_ref_channel=True)       # [F, C, C]
    assert torch.equal(one, w[1]) and ref_one.tolist() == [ref64[1]]


# ---- edge cases ------------------------------------------------------------------------------------------------------------------------------
def test_bins_with_an_all_zero_mask():
    from padertorch_amd import ops
    shape = (2, 3, 33, 65)
    Y, speech, noise = make_inputs(shape, seed=1)
    noise[:, :, :, 5] = 0                      # Phi_n = 0 in bin 5: w = 0, Z = 0
    speech[:, :, :, 9] = 0                     # Phi_s = 0 / 1e-10 = 0 in bin 9
    Yd, sd, nd = dev_tensor(Y), dev_tensor(speech), dev_tensor(noise)
    psd_s, psd_n = ops.get_power_spectral_density_matrix(Yd, sd), ops.get_power_spectral_density_matrix(Yd, nd)
    assert not bool(psd_n[:, 5].abs().any()) and not bool(psd_s[:, 9].abs().any())
    w, ref = ops.get_mvdr_vector_souden(psd_s, psd_n, return_ref_channel=True)
    Z = ops.mask_beamforming(Yd, sd, nd)
    for x in (psd_s, psd_n, w, Z):
        assert bool(torch.isfinite(torch.view_as_real(x)).all())
    assert not bool(w[:, 5].abs().any()) and not bool(Z[:, :, 5].abs().any())
    assert not bool(w[:, 9].abs().any()) and not bool(Z[:, :, 9].abs().any())
    assert bool(Z[:, :, 6].abs().all())
    ms, mn = ref_median(speech), ref_median(noise)
    Y64 = Y.astype(np.complex128)
    want_s, want_n = ref_psd(Y64, ms.astype(np.float64)), ref_psd(Y64, mn.astype(np.float64))
    assert deviation(host(psd_s), want_s) <= FACTOR * deviation(ref_psd(Y, ms), want_s)
    chosen = ref.tolist()
    for b in range(2):                         # the vector for the channel the device chose (the rank-one target makes the channels tie)
        want = ref_souden(want_s[b:b + 1], want_n[b:b + 1], chosen[b])[0]
        single = ref_souden(ref_psd(Y, ms)[b:b + 1], ref_psd(Y, mn)[b:b + 1], chosen[b])[0]
        assert deviation(host(w[b:b + 1]), want) <= FACTOR * deviation(single, want)


def test_jensheit_beamforming_returns_the_three_signals():
    from padertorch_amd.contrib.jensheit.evaluation import beamforming
    shape = (1, 3, 33, 65)
    Y, speech, noise = make_inputs(shape, seed=2)
    rng = np.random.default_rng(3)
    image, rest = cnormal(rng, *shape).astype(np.complex64), cnormal(rng, *shape).astype(np.complex64)
    ms, mn = ref_median(speech), ref_median(noise)

    def restate(cast_c, cast_r):
        Yc = Y.astype(cast_c)
        Ps, Pn = ref_psd(Yc, ms.astype(cast_r)), ref_psd(Yc, mn.astype(cast_r))
        return Ps, Pn
    Ps, Pn = restate(np.complex128, np.float64)
    got = beamforming(*(dev_tensor(x[0]) for x in (Y, speech, noise, image, rest)))               # CxTxF, as the reference's caller
    assert [tuple(g.shape) for g in got] == [(33, 65)] * 3
    # the channel is the device's choice (rank-one target: the candidates tie); recover it from the restatement's candidates
    cands = [ref_souden(Ps, Pn, r)[0] for r in range(3)]
    r = int(np.argmin([deviation(host(got[0])[None], ref_apply(w, Y.astype(np.complex128))) for w in cands]))
    w32 = ref_souden(*restate(np.complex64, np.float32), r)[0]
    for g, x in zip(got, (Y, image, rest)):
        want = ref_apply(cands[r], x.astype(np.complex128))
        tol = FACTOR * deviation(ref_apply(w32, x), want)
        err = deviation(host(g)[None], want)
        print(f'\njensheit: {err:.2e} (tol {tol:.2e})')
        assert err <= tol
    only = beamforming(*(dev_tensor(x) for x in (Y, speech, noise)))                                # ...xCxTxF, no images
    assert only[1] is None and only[2] is None and torch.equal(only[0][0], got[0])


# ---- SimpleMaskEstimator.enhance ----------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def estimator():
    from padertorch_amd import ops
    from padertorch_amd.contrib.examples.speech_enhancement.mask_estimator.model import SimpleMaskEstimator
    torch.manual_seed(0)
    net = SimpleMaskEstimator(65, num_units=32).cuda()
    y = torch.randn(2, 3, 2000, generator=torch.Generator().manual_seed(1)).cuda()
    y = y + y[:, :1].roll(3, -1)                                          # something the channels share
    return net, ops.STFT(128, 32), y


def test_enhance_is_stft_model_beamformer_istft():
    from padertorch_amd import ops
    net, stft, y = estimator()
    N = y.shape[-1]
    out = net.enhance(y, stft=stft, ref_channel=1)
    assert net.training and set(out) == {'masked', 'beamformed'}
    assert all(len(v) == 2 and all(x.shape == (N,) and x.is_cuda for x in v) for v in out.values())
    net.eval()
    with torch.no_grad():
        Y = stft(y)
        masks = net(dict(observation_abs=Y.abs().reshape(6, *Y.shape[2:])))
    net.train()
    speech, noise = (masks[f'{k}_mask_prediction'].reshape(Y.shape).contiguous() for k in ('speech', 'noise'))
    assert torch.equal(torch.stack(out['masked']), stft.inverse(speech[:, 0] * Y[:, 0])[..., :N])
    Z = ops.mask_beamforming(Y, speech, noise, ref_channel=1)
    assert torch.equal(torch.stack(out['beamformed']), stft.inverse(Z)[..., :N])
    Yh, sh, nh = host(Y), host(speech), host(noise)
    ms, mn = ref_median(sh), ref_median(nh)
    want = chain(Yh.astype(np.complex128), ms.astype(np.float64), mn.astype(np.float64), None, 1)['Z']
    tol = FACTOR * deviation(chain(Yh, ms, mn, None, 1)['Z'], want)
    err = deviation(host(Z), want)
    print(f'\nenhance: beamformed spectrum {err:.2e} (tol {tol:.2e})')
    assert err <= tol
    auto = net.enhance(y, stft=stft)                                      # the channel chosen on the device
    assert all(bool(torch.isfinite(x).all()) and x.shape == (N,) for x in auto['beamformed'])
    assert torch.equal(torch.stack(auto['masked']), torch.stack(out['masked']))


def test_enhance_runs_a_list_of_two_lengths_example_by_example():
    net, stft, y = estimator()
    both = net.enhance([y[0], y[1, :, :1500]], stft=stft, ref_channel=1)
    assert [tuple(x.shape) for x in both['beamformed']] == [(2000,), (1500,)] == [tuple(x.shape) for x in both['masked']]
    for k in both:
        assert torch.equal(both[k][0], net.enhance(y[:1], stft=stft, ref_channel=1)[k][0])
        assert torch.equal(both[k][1], net.enhance(y[1:, :, :1500], stft=stft, ref_channel=1)[k][0])
    padded = net.enhance(y, num_samples=[2000, 1500], stft=stft, ref_channel=1)
    for k in both:
        assert all(torch.equal(a, b) for a, b in zip(padded[k], both[k]))


def test_enhance_of_a_batch_does_not_synchronise():
    """The batched call is captured into a graph once (a host synchronisation between STFT and iSTFT would end the capture with an
    error) and the replay gives the eager result."""
    from padertorch_amd.ops import capture
    net, stft, y = estimator()
    eager = net.enhance(y, stft=stft)
    static = y.clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        net.enhance(static, stft=stft)                                    # warm-up on the capture stream
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with capture.capture_mode():
        with torch.cuda.graph(graph, stream=side):
            capture.zero_block(static.device)
            captured = net.enhance(static, stft=stft)
    graph.replay()
    torch.cuda.synchronize()
    for k in eager:
        assert all(torch.equal(a, b) for a, b in zip(captured[k], eager[k])), k
