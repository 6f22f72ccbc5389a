"""GEV and PCA beamforming with blind analytic normalization and phase correction on the GPU (``csrc/beamform.hip`` through
``ops.beamforming``) against the fp64 numpy restatement of ``tests/test_gev_host.py`` on the inputs of
``tests/test_gpu_beamforming.py``.

Error measure: max abs deviation over the max abs value of the fp64 result, over EVERY element.  Tolerance, per case and quantity: the
larger of 8 times the deviation of the same restatement run in complex64 / float32 from its fp64 run (never anything the kernels
produce) and ``2^-22`` (the vectors are stored as complex64, ``2^-24`` per part; for ``C = 1`` the single-precision BAN is exact and
the first value would be zero).  The gauge jumps where the two largest components of a vector tie, so every case first asserts on the
fp64 restatement alone that their magnitude ratio is at least ``1 + 1e-4`` in every bin (a shape that misses it gets another seed,
never another threshold).  A case is computed once (restatement and kernels) and shared by the tests that look at it.

Quantities: ``gev`` / ``pca`` the plain vectors, ``*_lambda`` their eigenvalues, ``*_ban`` the normalized vectors, ``*_phase`` the
vector ``mask_beamforming`` applies (``phase(ban(gev))`` for ``'gev+ban'``, ``phase(pca)`` for ``'pca'``), ``*_Z`` the output.
"""
import functools

import numpy as np
import pytest
import torch

from test_gev_host import ref_apply, ref_ban, ref_gev, ref_median, ref_pca, ref_phase, ref_psd, top_two_ratio
from test_gpu_beamforming import FACTOR, dev_tensor, deviation, host, make_inputs

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1, 9, 5), (2, 2, 9, 65), (2, 3, 33, 65), (3, 6, 70, 129), (2, 5, 24, 300), (1, 4, 40, 257), (2, 7, 20, 33), (1, 8, 130, 67)]
FRAMES = {(3, 6, 70, 129): [70, 41, 12], (2, 5, 24, 300): [24, 9]}
SEEDS = {}                      # shape -> seed where seed 0 misses the gauge condition
FLOOR = 2. ** -22
MIN_RATIO = 1 + 1e-4


def chain(Y, ms, mn, frames):
    """The restatement in the precision of its inputs: every quantity the tests compare."""
    Ps, Pn = ref_psd(Y, ms, frames), ref_psd(Y, mn, frames)
    out = dict(psd_s=Ps, psd_n=Pn)
    out['gev'], out['gev_lambda'] = ref_gev(Ps, Pn)
    out['pca'], out['pca_lambda'] = ref_pca(Ps)
    out['gev_ban'], out['pca_ban'] = ref_ban(out['gev'], Pn), ref_ban(out['pca'], Pn)
    out['gev_phase'], out['pca_phase'] = ref_phase(out['gev_ban']), ref_phase(out['pca'])
    out['gev_Z'], out['pca_Z'] = ref_apply(out['gev_phase'], Y, frames), ref_apply(out['pca_phase'], Y, frames)
    return out


def run_kernels(Yd, sd, nd, fr):
    from padertorch_amd import ops
    got = dict(psd_s=ops.get_power_spectral_density_matrix(Yd, sd, frames=fr), psd_n=ops.get_power_spectral_density_matrix(Yd, nd, frames=fr))
    got['gev'], got['gev_lambda'] = ops.get_gev_vector(got['psd_s'], got['psd_n'], return_eigenvalue=True)
    got['pca'], got['pca_lambda'] = ops.get_pca_vector(got['psd_s'], return_eigenvalue=True)
    got['gev_ban'] = ops.blind_analytic_normalization(got['gev'], got['psd_n'])
    got['pca_ban'] = ops.blind_analytic_normalization(got['pca'], got['psd_n'])
    got['gev_phase'], got['pca_phase'] = ops.phase_correction(got['gev_ban']), ops.phase_correction(got['pca'])
    got['gev_Z'] = ops.apply_beamforming_vector(got['gev_phase'], Yd, frames=fr)
    got['pca_Z'] = ops.apply_beamforming_vector(got['pca_phase'], Yd, frames=fr)
    got['gev_Z_fused'] = ops.mask_beamforming(Yd, sd, nd, frames=fr, beamformer='gev+ban')
    got['pca_Z_fused'] = ops.mask_beamforming(Yd, sd, nd, frames=fr, beamformer='pca')
    return got


@functools.lru_cache(maxsize=None)
def restatement(shape):
    """Inputs, the fp64 restatement and the tolerances from its single-precision run: once per shape, no GPU."""
    Y, speech, noise = make_inputs(shape, SEEDS.get(shape, 0))
    frames = FRAMES.get(shape)
    ms, mn = ref_median(speech), ref_median(noise)                      # float32, exactly what the kernel takes
    want = chain(Y.astype(np.complex128), ms.astype(np.float64), mn.astype(np.float64), frames)
    single = chain(Y, ms, mn, frames)
    assert all(v.dtype in (np.complex64, np.float32) for v in single.values()), {k: v.dtype for k, v in single.items()}
    tol = {k: max(FACTOR * deviation(single[k], want[k]), FLOOR) for k in want}
    return dict(inputs=(Y, speech, noise), frames=frames, want=want, tol=tol)


@functools.lru_cache(maxsize=None)
def case(shape):
    c = dict(restatement(shape))
    fr = None if c['frames'] is None else torch.tensor(c['frames'], dtype=torch.int32).cuda()
    c['device'] = (*(dev_tensor(x) for x in c['inputs']), fr)
    c['got'] = run_kernels(*c['device'])
    return c


@pytest.mark.parametrize('shape', SHAPES, ids=str)
def test_vectors_eigenvalues_and_output_against_the_restatement(shape):
    want = restatement(shape)['want']
    if shape[1] > 1:                                                      # a condition on the inputs, not a measurement
        ratios = {k: float(top_two_ratio(want[k]).min()) for k in ('gev', 'pca')}
        print(f'\n{shape} smallest ratio of the two largest components: {ratios}')
        assert min(ratios.values()) >= MIN_RATIO, ratios
    c = case(shape)
    errors = {k: deviation(host(c['got'][k]), want[k]) for k in want}
    for k in ('gev_Z', 'pca_Z'):
        errors[k + '_fused'] = deviation(host(c['got'][k + '_fused']), want[k])
    values = np.sort(np.linalg.eigvalsh(want['psd_s']), -1)
    print(f'{shape} cond(Phi_n) <= {np.linalg.cond(want["psd_n"]).max():.1f}, PCA eigenvalue gap ratio >= '
          f'{(values[..., -1] / np.maximum(values[..., -2 if shape[1] > 1 else -1], 1e-300)).min():.3f}: '
          + ', '.join(f'{k} {e:.2e} (tol {c["tol"][k.replace("_fused", "")]:.2e})' for k, e in errors.items()))
    for k, e in errors.items():
        assert e <= c['tol'][k.replace('_fused', '')], (k, e, c['tol'][k.replace('_fused', '')])
    got = c['got']
    assert got['gev'].dtype == got['pca_ban'].dtype == got['gev_phase'].dtype == got['gev_Z'].dtype == torch.complex64
    assert got['gev_lambda'].dtype == got['pca_lambda'].dtype == torch.float64 and got['gev_lambda'].shape == (shape[0], shape[3])


@pytest.mark.parametrize('shape', SHAPES, ids=str)
def test_separate_functions_equal_the_fused_chain_and_runs_are_bit_identical(shape):
    from padertorch_amd import ops
    got = case(shape)['got']
    Yd, sd, nd, fr = case(shape)['device']
    assert torch.equal(got['gev_Z'], got['gev_Z_fused']) and torch.equal(got['pca_Z'], got['pca_Z_fused'])
    Ps, Pn = got['psd_s'], got['psd_n']
    assert torch.equal(ops.get_bf_vector('gev', Ps, Pn), got['gev']) and torch.equal(ops.get_bf_vector('pca', Ps, Pn), got['pca'])
    fused = ops.get_bf_vector('gev+ban', Ps, Pn)                          # BAN inside the eigen launch
    assert torch.equal(fused, got['gev_ban']) and torch.equal(ops.get_bf_vector('pca+ban', Ps, Pn), got['pca_ban'])
    assert torch.equal(ops.phase_correction(fused), got['gev_phase'])    # the public function and the chain's: the same launch
    souden = ops.get_mvdr_vector_souden(Ps, Pn, 0)
    assert torch.equal(ops.get_bf_vector('mvdr_souden+ban', Ps, Pn, ref_channel=0), ops.blind_analytic_normalization(souden, Pn))
    assert torch.equal(ops.get_bf_vector('mvdr_souden', Ps, Pn, ref_channel=0), souden)
    for k, beamformer in (('gev_Z', 'gev+ban'), ('pca_Z', 'pca')):        # a second run
        assert torch.equal(ops.mask_beamforming(Yd, sd, nd, frames=fr, beamformer=beamformer), got[k])
    again = ops.get_gev_vector(Ps, Pn, return_eigenvalue=True)
    assert torch.equal(again[0], got['gev']) and torch.equal(again[1], got['gev_lambda'])
    one = ops.get_gev_vector(Ps[0], Pn[0], return_eigenvalue=True)       # [F, C, C]
    assert torch.equal(one[0], got['gev'][0]) and torch.equal(one[1], got['gev_lambda'][0])
    assert torch.equal(ops.phase_correction(got['pca'][0]), got['pca_phase'][0])
    assert torch.equal(ops.blind_analytic_normalization(got['pca'][0], Pn[0]), got['pca_ban'][0])


@pytest.mark.parametrize('shape', SHAPES, ids=str)
def test_normalisations(shape):
    """``w^H Phi_n w = 1`` (GEV) and ``|w| = 1`` (PCA) to 1e-6 on the stored complex64 vectors; the gauge component is real, positive."""
    got = case(shape)['got']
    w, Pn = host(got['gev']).astype(np.complex128), host(got['psd_n'])
    assert np.abs(np.einsum('bfd,bfde,bfe->bf', w.conj(), Pn, w) - 1).max() <= 1e-6
    assert np.abs(np.linalg.norm(host(got['pca']).astype(np.complex128), axis=-1) - 1).max() <= 1e-6
    for k in ('gev', 'pca', 'gev_ban', 'pca_ban'):
        v = host(got[k])
        top = np.take_along_axis(v, np.abs(v).argmax(-1)[..., None], -1)
        assert (top.imag == 0).all() and (top.real > 0).all(), k
    aligned = host(got['gev_phase']).astype(np.complex128)
    d = (aligned[:, 1:] * aligned[:, :-1].conj()).sum(-1)                 # neighbours in phase: real, positive
    norms = np.linalg.norm(aligned, axis=-1)
    assert (d.real > 0).all() and (np.abs(d.imag) <= 1e-6 * norms[:, 1:] * norms[:, :-1]).all()


def test_the_default_is_the_souden_path_bit_for_bit():
    from padertorch_amd import ops
    Yd, sd, nd, fr = case((3, 6, 70, 129))['device']
    default = ops.mask_beamforming(Yd, sd, nd, frames=fr)
    assert torch.equal(default, ops.mask_beamforming(Yd, sd, nd, frames=fr, beamformer='mvdr_souden'))
    Ps, Pn = case((3, 6, 70, 129))['got']['psd_s'], case((3, 6, 70, 129))['got']['psd_n']
    assert torch.equal(default, ops.apply_beamforming_vector(ops.get_mvdr_vector_souden(Ps, Pn), Yd, frames=fr))
    assert not torch.equal(default, case((3, 6, 70, 129))['got']['gev_Z'])


def test_frames_hide_what_lies_behind_them():
    from padertorch_amd import ops
    for shape in FRAMES:
        c = case(shape)
        Y, speech, noise = (x.copy() for x in c['inputs'])
        for b, n in enumerate(c['frames']):
            Y[b, :, n:] = 1e30 * (1 + 1j)
            speech[b, :, n:] = np.nan
            noise[b, :, n:] = np.nan
        fr = c['device'][3]
        for k, beamformer in (('gev_Z', 'gev+ban'), ('pca_Z', 'pca')):
            Z = ops.mask_beamforming(dev_tensor(Y), dev_tensor(speech), dev_tensor(noise), frames=fr, beamformer=beamformer)
            assert torch.equal(Z, c['got'][k]), (shape, k)
            for b, n in enumerate(c['frames']):
                assert not bool(Z[b, n:].abs().any()) and bool(Z[b, :n].abs().any())


def test_bins_with_an_all_zero_noise_mask():
    from padertorch_amd import ops
    shape, bins = (2, 3, 33, 65), [0, 5, 40]
    c = case(shape)
    Y, speech, noise = (x.copy() for x in c['inputs'])
    noise[:, :, :, bins] = 0                                              # Phi_n = 0: no Cholesky factor
    Yd, sd, nd = dev_tensor(Y), dev_tensor(speech), dev_tensor(noise)
    Ps, Pn = ops.get_power_spectral_density_matrix(Yd, sd), ops.get_power_spectral_density_matrix(Yd, nd)
    others = [f for f in range(shape[3]) if f not in bins]
    for name in ('gev', 'gev+ban'):
        w = ops.get_bf_vector(name, Ps, Pn)
        assert not bool(w[:, bins].abs().any()) and bool(torch.isfinite(torch.view_as_real(w)).all())
        assert torch.equal(w[:, others], c['got']['gev' if name == 'gev' else 'gev_ban'][:, others])       # the same gauge elsewhere
        Z = ops.mask_beamforming(Yd, sd, nd, beamformer=name)
        assert bool(torch.isfinite(torch.view_as_real(Z)).all())
        assert not bool(Z[:, :, bins].abs().any()) and bool(Z[:, :, others].abs().sum(1).all())
    w, lam = ops.get_gev_vector(Ps, Pn, return_eigenvalue=True)
    assert not bool(lam[:, bins].any()) and bool((lam[:, others] > 0).all())
    want = ref_phase(host(ops.get_bf_vector('gev+ban', Ps, Pn)).astype(np.complex128))                  # the chain starts again behind a gap
    assert deviation(host(ops.phase_correction(ops.get_bf_vector('gev+ban', Ps, Pn))), want) <= FLOOR
    pca = ops.get_bf_vector('pca+ban', Ps, Pn)                            # BAN with a zero Phi_n: 0 / tiny
    assert not bool(pca[:, bins].abs().any()) and torch.equal(pca[:, others], c['got']['pca_ban'][:, others])


def test_a_captured_chain_replays_on_new_contents():
    from padertorch_amd import ops
    shape = (2, 3, 33, 65)
    first = [dev_tensor(x) for x in make_inputs(shape, seed=5)]
    static = [x.clone() for x in first]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.mask_beamforming(*static, beamformer='gev+ban')              # warm-up on the capture stream
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):                            # (a synchronisation or a host read would end the capture)
        captured = ops.mask_beamforming(*static, beamformer='gev+ban')
    for s, x in zip(static, case(shape)['device'][:3]):
        s.copy_(x)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(captured, case(shape)['got']['gev_Z'])
    assert not torch.equal(captured, ops.mask_beamforming(*first, beamformer='gev+ban'))


def test_enhance_with_the_gev_beamformer():
    from test_gpu_beamforming import estimator
    net, stft, y = estimator()
    souden = net.enhance([y[0], y[1, :, :1500]], stft=stft)
    net.beamformer = 'gev+ban'
    try:
        out = net.enhance([y[0], y[1, :, :1500]], stft=stft)
        with pytest.raises(ValueError, match='ref_channel is for mvdr_souden only'):
            net.enhance(y, stft=stft, ref_channel=1)
    finally:
        del net.beamformer                                                # the class default again: the estimator is shared
    assert net.beamformer == 'mvdr_souden' and net.training
    assert [tuple(x.shape) for x in out['beamformed']] == [(2000,), (1500,)]
    assert all(bool(torch.isfinite(x).all()) and bool(x.abs().any()) for x in out['beamformed'])
    assert all(torch.equal(a, b) for a, b in zip(out['masked'], souden['masked']))
    assert not any(torch.equal(a, b) for a, b in zip(out['beamformed'], souden['beamformed']))


def test_jensheit_beamforming_with_the_gev_and_pca_vectors():
    from padertorch_amd import ops
    from padertorch_amd.contrib.jensheit.evaluation import beamforming
    c = case((2, 3, 33, 65))
    Yd, sd, nd, _ = c['device']
    image = dev_tensor(make_inputs((2, 3, 33, 65), seed=7)[0])
    for get_bf_fn, k in ((ops.get_gev_vector, 'gev'), (ops.get_pca_vector, 'pca')):
        out = beamforming(Yd, sd, nd, speech_image=image, get_bf_fn=get_bf_fn)                      # the plain vector: no phase correction
        assert out[2] is None and torch.equal(out[0], ops.apply_beamforming_vector(c['got'][k], Yd))
        assert torch.equal(out[1], ops.apply_beamforming_vector(c['got'][k], image))
