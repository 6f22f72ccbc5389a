"""Fast Griffin-Lim phase retrieval with momentum (FGLA) on the HIP STFT kernels.

Drop-in for ``padertorch/contrib/mk/synthesis/parametric/griffin_lim.py`` (``griffin_lim_step`` :32-74, ``fast_griffin_lim`` :77-156,
``FGLA`` :159-214) for torch tensors on an MI355X and ``padertorch_amd.ops.STFT``.  The reference's numpy / ``paderbox`` backend does
not exist here: a numpy ``a`` or a ``paderbox`` STFT is refused.

One iteration is ``istft_kernel``, one update launch and a one-workgroup launch that owns the RMSE history and the stop
(``ops/griffin_lim.py``, DESIGN.md "Griffin-Lim"); the stop is device data, so ``fast_griffin_lim(..., x=given)`` can be captured in a
``torch.cuda.graph``.  Arithmetic is fp32 whatever the dtype of ``a`` (the documented deviation of ``ops.STFT``); the result is cast
back to ``a``'s dtype.

[1]: Peer, Welker, Gerkmann: "Beyond Griffin-Lim: Improved Iterative Phase Retrieval for Speech", IWAENC 2022.
"""
import math
import typing

import numpy as np
import torch

from ..... import _lib
from .....data import example_to_device
from .....ops import griffin_lim as _gl
from .....ops._stft import STFT, _IstftFn, _StftFn
from ..base import Synthesis

__all__ = ['fast_griffin_lim', 'griffin_lim_step', 'FGLA']

_NUMPY_BACKEND = ('the numpy / paderbox backend of the reference\'s Griffin-Lim does not exist in padertorch_amd: pass a torch tensor '
                  'on the GPU and a padertorch_amd.ops.STFT')


def _check_backend(a, stft):
    if isinstance(a, np.ndarray) or not isinstance(a, torch.Tensor):
        raise TypeError(f'a is a {type(a).__name__}: {_NUMPY_BACKEND}')
    if not isinstance(stft, STFT):
        raise TypeError(f'stft is a {type(stft).__module__}.{type(stft).__name__}: {_NUMPY_BACKEND}')
    _lib.require_gpu(a)
    assert a.is_floating_point(), a.dtype
    F = stft.size // 2 + 1
    assert a.dim() >= 2 and a.shape[-1] == F, f'a must be [..., frames, {F}] for an STFT of size {stft.size}, not {tuple(a.shape)}'


def _rows(a):
    """``[..., frames, F]`` any float dtype -> ``[rows, frames, F]`` float32 contiguous (differentiable)."""
    return a.reshape(-1, *a.shape[-2:]).to(torch.float32).contiguous()


def _interleaved(z, shape):
    """A complex tensor of ``shape [..., frames, F]`` -> its ``[rows, frames, F, 2]`` float32 view / copy."""
    assert z.is_complex() and tuple(z.shape) == tuple(shape), (z.dtype, tuple(z.shape), tuple(shape))
    return torch.view_as_real(z.detach().reshape(-1, *shape[-2:]).to(torch.complex64).contiguous())


def _inverse(spec, stft, lead, dtype):
    """Interleaved ``[rows, frames, F, 2]`` -> signal ``[*lead, T]`` in ``dtype``."""
    audio = _IstftFn.apply(spec, stft, 0)
    return audio.reshape(*lead, audio.shape[-1]).to(dtype)


def griffin_lim_step(a, reconstruction_stft, stft: STFT):
    """One Griffin-Lim projection pair: ``P = a exp(j angle(reconstruction_stft))`` (onto the magnitudes), ``audio = stft.inverse(P)``,
    ``stft_signal = stft(audio)`` (onto the consistent spectra).

    Returns ``(stft_signal, audio)``; ``stft_signal`` is complex whatever ``stft.complex_representation`` is.
    """
    _check_backend(a, stft)
    _lib.require_gpu(reconstruction_stft)
    lead, frames = a.shape[:-2], a.shape[-2]
    _gl.round_trip_samples(stft, frames)
    P = _gl.gl_project(_rows(a), _interleaved(reconstruction_stft, a.shape))
    audio = _IstftFn.apply(P, stft, 0)
    spec = torch.view_as_complex(_StftFn.apply(audio, stft, 0, None))
    spec = spec.reshape(*lead, *spec.shape[-2:])
    audio = audio.reshape(*lead, audio.shape[-1]).to(a.dtype)
    return (spec.to(torch.complex128) if a.dtype == torch.float64 else spec), audio


def fast_griffin_lim(a, stft: STFT, alpha=0.95, iterations=100, atol: float = 0.1, verbose=False, x=None, *, generator=None,
                     return_info=False):
    """Griffin-Lim with momentum [1]: a waveform whose STFT magnitude approximates ``a``.

    Args:
        a: magnitude spectrogram ``[..., frames, stft.size // 2 + 1]`` on the GPU, any float dtype
        stft: the ``padertorch_amd.ops.STFT`` the magnitudes belong to (any ``complex_representation``)
        alpha: momentum, ``0 <= alpha <= 1``
        iterations: at most this many iterations (0: only the final inverse)
        atol: stop behind the first iteration whose RMSE between ``|x|`` and ``a`` (over the whole tensor) is below it
        verbose: print the RMSE of every iteration that ran (after the loop, one synchronisation)
        x: complex64 start whose angle is used; None: a random phase, uniform in [-pi, pi), drawn on ``a``'s device
        generator: the ``torch.Generator`` (on ``a``'s device) of the random phase
        return_info: also return ``ops.griffin_lim.GriffinLimInfo(rmse, num_iterations, x)`` (device tensors)

    Returns: the signal ``[..., T]`` in ``a``'s dtype.  If ``a`` requires a gradient it flows through the last projection and the
    inverse STFT; the phase is a constant.
    """
    _check_backend(a, stft)
    iterations = int(iterations)
    assert iterations >= 0, iterations
    lead, frames = a.shape[:-2], a.shape[-2]
    _gl.round_trip_samples(stft, frames)
    a32 = _rows(a)
    a_const = a32.detach()
    with torch.no_grad():
        if x is None:
            angle = torch.rand(a_const.shape, generator=generator, device=a.device, dtype=torch.float32) * (2 * math.pi) - math.pi
            y0 = torch.stack((torch.cos(angle), torch.sin(angle)), dim=-1)
        else:
            if isinstance(x, np.ndarray):
                raise TypeError(f'x is a numpy array: {_NUMPY_BACKEND}')
            assert x.dtype in (torch.complex64,), x.dtype
            _lib.require_gpu(x)
            y0 = _interleaved(x, a.shape)
        xbuf = torch.ops.ptmi.gl_project(a_const, y0)       # x = a exp(j angle)
        P = xbuf.clone()                                    # y = x: its projection is x itself
        info = _gl.gl_iterations(a_const, xbuf, P, stft, alpha, iterations, atol)
    signal = _inverse(_gl.gl_project(a32, xbuf), stft, lead, a.dtype)
    if verbose:
        rmse, ran = info.rmse.cpu(), int(info.num_iterations)
        for n in range(ran):
            print('Reconstruction iteration: {}/{} RMSE: {} '.format(n, iterations, rmse[n]))
    if return_info:
        return signal, _gl.GriffinLimInfo(info.rmse, info.num_iterations, info.x.reshape(*lead, *info.x.shape[-2:]))
    return signal


class FGLA(Synthesis):
    """Phase reconstruction with :func:`fast_griffin_lim`."""

    def __init__(self, sampling_rate: int, stft: STFT, alpha: float = .95, iterations: int = 30, atol: float = 0.1):
        """
        Args:
            sampling_rate: sampling rate of the synthesised signal
            stft: the STFT that produced the magnitude spectrograms
            alpha, iterations, atol: see :func:`fast_griffin_lim`
        """
        super().__init__()
        self.sampling_rate = sampling_rate
        self.stft = stft
        self.alpha = alpha
        self.iterations = iterations
        self.atol = atol

    def __call__(self, mag_spec, sequence_lengths: typing.Optional[typing.List[int]] = None,
                 target_sampling_rate: typing.Optional[int] = None):
        """``mag_spec [..., frames, stft.size // 2 + 1]`` (a numpy array is moved to the GPU) -> waveform tensor.  ``sequence_lengths`` is
        ignored like in the reference; a ``target_sampling_rate`` other than ``sampling_rate`` raises ``NotImplementedError``."""
        del sequence_lengths
        self._resample(None, target_sampling_rate)          # refuse before the work, not after
        if isinstance(mag_spec, np.ndarray):
            mag_spec = example_to_device(mag_spec, torch.device('cuda'))
        signal = fast_griffin_lim(mag_spec, self.stft, self.alpha, self.iterations, self.atol)
        return self._resample(signal, target_sampling_rate)
