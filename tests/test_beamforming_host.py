"""Mask-based MVDR beamforming (``ops.beamforming``, ``csrc/beamform.hip``) without a GPU: the fp64 restatement the GPU tests compare
against (numpy, the formulas of the ``ops.beamforming`` docstring; ``tests/test_gpu_beamforming.py`` imports it from here) checked on
closed forms, and the interface's registration and argument checks."""
import ast
import inspect
from pathlib import Path

import numpy as np
import pytest
import torch

from padertorch_amd import ops
from padertorch_amd.contrib.jensheit import evaluation
from padertorch_amd.ops import beamforming as bf

REFERENCE = Path('/root/reference/padertorch/contrib/jensheit/evaluation.py')


# ---- the restatement: every function computes in the precision of its inputs (complex128 / float64, or complex64 / float32) ----------
def ref_median(mask):
    """``[B, C, T, F]`` -> ``[B, T, F]``: numpy's median over the channels."""
    return np.median(mask, axis=1)


def ref_psd(Y, m=None, frames=None, normalize=True):
    """``Y [B, C, T, F]``, ``m [B, T, F]`` (None: ones) -> ``Phi [B, F, C, C]``; frames ``t >= frames[b]`` do not count."""
    B, C, T, F = Y.shape
    real = Y.real.dtype
    valid = np.arange(T)[None] < (np.full(B, T) if frames is None else np.asarray(frames))[:, None]
    m = np.where(valid[:, :, None], np.ones((B, T, F), real) if m is None else m, 0).astype(real)
    Y = np.where(valid[:, None, :, None], Y, 0).astype(Y.dtype)
    psd = np.einsum('btf,bdtf,betf->bfde', m, Y, Y.conj())
    if normalize:
        psd = psd / np.maximum(m.sum(1), real.type(1e-10))[:, :, None, None]
    return psd


def ref_solve(A, R):
    """``A^-1 R`` for ``[N, C, C]`` stacks: Gaussian elimination, partial pivoting by ``|re| + |im|`` (first maximum); a pivot that is
    exactly zero leaves the unknowns of its column zero."""
    A, X = A.copy(), R.copy()
    N, C, _ = A.shape
    n, one = np.arange(N), A.dtype.type(1)
    zero = np.zeros((N, C), bool)
    for k in range(C):
        mag = np.abs(A[:, k:, k].real) + np.abs(A[:, k:, k].imag)
        p, z = k + mag.argmax(1), mag.max(1) == 0
        zero[:, k] = z
        for M in (A, X):
            M[n, k], M[n, p] = M[n, p].copy(), M[n, k].copy()
        factor = np.where(z[:, None], 0, A[:, k + 1:, k] / np.where(z, one, A[:, k, k])[:, None]).astype(A.dtype)
        A[:, k + 1:] -= factor[:, :, None] * A[:, k:k + 1]
        X[:, k + 1:] -= factor[:, :, None] * X[:, k:k + 1]
    for k in reversed(range(C)):
        s, z = X[:, k] - np.einsum('nj,njc->nc', A[:, k, k + 1:], X[:, k + 1:]), zero[:, k, None]
        X[:, k] = np.where(z, 0, s / np.where(z, one, A[:, k, k, None])).astype(A.dtype)
    return X


def ref_souden(Ps, Pn, ref_channel=None):
    """``[B, F, C, C]`` PSD matrices -> ``(w [B, F, C], ref [B], ratio [B, C])``."""
    B, F, C, _ = Ps.shape
    tiny = np.finfo(Ps.real.dtype).tiny
    X = ref_solve(Pn.reshape(-1, C, C), Ps.reshape(-1, C, C)).reshape(B, F, C, C)
    M = X / np.maximum(np.trace(X, axis1=-2, axis2=-1).real, tiny)[..., None, None]
    num = np.einsum('bfdr,bfde,bfer->br', M.conj(), Ps, M).real
    den = np.einsum('bfdr,bfde,bfer->br', M.conj(), Pn, M).real
    ratio = num / np.maximum(den, tiny)
    ref = ratio.argmax(1) if ref_channel is None else np.full(B, ref_channel)
    return M[np.arange(B), :, :, ref], ref, ratio


def ref_apply(w, X, frames=None):
    """``w [B, F, C]``, ``X [B, C, T, F]`` -> ``Z [B, T, F]``, zero behind ``frames[b]``."""
    Z = np.einsum('bfc,bctf->btf', w.conj(), X)
    if frames is not None:
        Z[np.arange(X.shape[2])[None] >= np.asarray(frames)[:, None]] = 0
    return Z


# ---- the restatement against closed forms ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('C,ref', [(1, 0), (2, 1), (3, 0), (6, 4), (8, 7)])
def test_restatement_is_distortionless_on_a_rank_one_target(C, ref):
    rng = np.random.default_rng(C)
    F = 5
    a = rng.standard_normal((1, F, C)) + 1j * rng.standard_normal((1, F, C))
    sigma = rng.uniform(0.5, 2, (1, F))
    Ps = sigma[..., None, None] * a[..., :, None] * a[..., None, :].conj()
    Pn = np.broadcast_to(np.eye(C, dtype=np.complex128), Ps.shape).copy()
    w, chosen, _ = ref_souden(Ps, Pn, ref)
    want = a * a[..., ref:ref + 1].conj() / (np.abs(a) ** 2).sum(-1, keepdims=True)
    assert np.abs(w - want).max() <= 1e-12 and chosen.tolist() == [ref]
    assert np.abs(np.einsum('bfc,bfc->bf', w.conj(), a) - a[..., ref]).max() <= 1e-12          # w^H a = a_ref


def test_restatement_solves_with_pivoting_and_gives_zero_for_a_zero_noise_matrix():
    rng = np.random.default_rng(0)
    A = rng.standard_normal((7, 4, 4)) + 1j * rng.standard_normal((7, 4, 4))
    A[:, 0, 0] = 0                                                                          # the first pivot has to be swapped in
    R = rng.standard_normal((7, 4, 4)) + 1j * rng.standard_normal((7, 4, 4))
    assert np.abs(ref_solve(A, R) - np.linalg.solve(A, R)).max() <= 1e-12
    Ps = (R @ R.conj().transpose(0, 2, 1))[None]
    w, _, _ = ref_souden(Ps, np.zeros_like(Ps), 2)
    assert w.shape == (1, 7, 4) and not w.any()
    w, _, _ = ref_souden(Ps, np.zeros_like(Ps))
    assert not w.any() and np.isfinite(w).all()


def test_restatement_median_of_an_even_channel_count_and_psd():
    mask = np.array([0.1, 0.9, 0.4, 0.2], np.float32).reshape(1, 4, 1, 1)
    assert ref_median(mask).item() == np.float32(np.float32(0.2) + np.float32(0.4)) / 2
    rng = np.random.default_rng(1)
    Y = rng.standard_normal((2, 3, 5, 4)) + 1j * rng.standard_normal((2, 3, 5, 4))
    m = rng.uniform(size=(2, 5, 4))
    psd = ref_psd(Y, m, frames=[5, 2])
    for b, n in ((0, 5), (1, 2)):
        for f in range(4):
            want = sum(m[b, t, f] * np.outer(Y[b, :, t, f], Y[b, :, t, f].conj()) for t in range(n)) / m[b, :n, f].sum()
            assert np.abs(psd[b, f] - want).max() <= 1e-12
    assert np.abs(ref_psd(Y, None, frames=[5, 2], normalize=False)[1] - ref_psd(Y[:, :, :2])[1] * 2).max() <= 1e-12
    assert not ref_psd(Y, np.zeros_like(m)).any()                                           # the 1e-10 guard: 0 / 1e-10


# ---- the interface ----------------------------------------------------------------------------------------------------------------------
def test_ops_are_registered_with_a_cuda_kernel_only():
    for n in ('bf_psd', 'bf_souden', 'bf_apply'):
        assert getattr(torch.ops.ptmi, n).default._schema.name == f'ptmi::{n}'
        assert torch._C._dispatch_has_kernel_for_dispatch_key(f'ptmi::{n}', 'CUDA')
        assert not torch._C._dispatch_has_kernel_for_dispatch_key(f'ptmi::{n}', 'CPU')
    for n in ('get_power_spectral_density_matrix', 'get_mvdr_vector_souden', 'apply_beamforming_vector', 'mask_beamforming'):
        assert getattr(ops, n) is getattr(bf, n)


def _inputs(C=3, T=4, F=5):
    Y = torch.zeros(2, C, T, F, dtype=torch.complex64)
    return Y, torch.ones(2, C, T, F), torch.ones(2, C, T, F)


def test_cpu_tensors_raise_the_no_fallback_error():
    Y, s, n = _inputs()
    psd = torch.zeros(2, 5, 3, 3, dtype=torch.complex128)
    for call in (lambda: bf.get_power_spectral_density_matrix(Y, s), lambda: bf.get_power_spectral_density_matrix(Y[0]),
                 lambda: bf.get_mvdr_vector_souden(psd, psd, 0), lambda: bf.apply_beamforming_vector(torch.zeros(2, 5, 3, dtype=torch.complex64), Y),
                 lambda: bf.mask_beamforming(Y, s, n), lambda: evaluation.beamforming(Y, s, n)):
        with pytest.raises(RuntimeError, match='no CPU fallback'):
            call()


def test_more_than_eight_channels_raise():
    Y, s, n = _inputs(C=9)
    psd = torch.zeros(5, 9, 9, dtype=torch.complex128)
    for call in (lambda: bf.mask_beamforming(Y, s, n), lambda: bf.get_power_spectral_density_matrix(Y, s),
                 lambda: bf.get_mvdr_vector_souden(psd, psd), lambda: bf.apply_beamforming_vector(torch.zeros(2, 5, 9, dtype=torch.complex64), Y)):
        with pytest.raises(NotImplementedError, match='at most 8 channels'):
            call()


def test_other_dtypes_raise():
    Y, s, n = _inputs()
    with pytest.raises(NotImplementedError, match='float32 only'):
        bf.mask_beamforming(Y, s.double(), n)
    with pytest.raises(NotImplementedError, match='float32 only'):
        bf.get_power_spectral_density_matrix(Y, s.double())
    with pytest.raises(NotImplementedError, match='complex64 only'):
        bf.get_power_spectral_density_matrix(Y.to(torch.complex128), s)
    with pytest.raises(NotImplementedError, match='complex128 only'):
        bf.get_mvdr_vector_souden(torch.zeros(5, 3, 3, dtype=torch.complex64), torch.zeros(5, 3, 3, dtype=torch.complex64))
    with pytest.raises(NotImplementedError, match='int32 only'):
        bf.get_power_spectral_density_matrix(Y, s, frames=torch.tensor([4, 2]))


def test_inputs_that_require_grad_raise():
    Y, s, n = _inputs()
    with pytest.raises(NotImplementedError, match='inference only'):
        bf.mask_beamforming(Y, s.requires_grad_(), n)
    with pytest.raises(NotImplementedError, match='inference only'):
        bf.apply_beamforming_vector(torch.zeros(2, 5, 3, dtype=torch.complex64), Y.clone().requires_grad_())


def test_shapes_are_checked():
    Y, s, n = _inputs()
    with pytest.raises(ValueError, match='mask of shape'):
        bf.get_power_spectral_density_matrix(Y, s[:, 0])                      # a reduced mask needs channel_reduce=None
    with pytest.raises(ValueError, match='channel_reduce'):
        bf.get_power_spectral_density_matrix(Y, s, channel_reduce='mean')
    with pytest.raises(ValueError, match='ref_channel'):
        bf.mask_beamforming(Y, s, n, ref_channel=3)


@pytest.mark.skipif(not REFERENCE.exists(), reason='the reference tree is not on this machine')
def test_jensheit_signature_is_the_references():
    tree = ast.parse(REFERENCE.read_text())
    fn = next(node for node in tree.body if isinstance(node, ast.FunctionDef) and node.name == 'beamforming')
    names = [a.arg for a in fn.args.args]
    ours = inspect.signature(evaluation.beamforming)
    assert list(ours.parameters) == names
    defaults = dict(zip(names[len(names) - len(fn.args.defaults):], fn.args.defaults))
    for name, p in ours.parameters.items():
        assert (p.default is inspect.Parameter.empty) == (name not in defaults)
        if name in defaults and isinstance(defaults[name], ast.Constant):
            assert p.default == defaults[name].value
    assert evaluation.__all__ == ['beamforming']


def test_enhance_checks_its_stft():
    from padertorch_amd.contrib.examples.speech_enhancement.mask_estimator.model import SimpleMaskEstimator
    me = SimpleMaskEstimator(65, num_units=32)
    assert list(inspect.signature(me.enhance).parameters) == ['y', 'num_samples', 'stft', 'ref_channel']
    with pytest.raises(ValueError, match='65 bins'):
        me.enhance(torch.zeros(1, 3, 2000), stft=ops.STFT(256, 64))
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        me.enhance(torch.zeros(1, 3, 2000), stft=ops.STFT(128, 32))
    assert me.training                                                         # the mode is put back
