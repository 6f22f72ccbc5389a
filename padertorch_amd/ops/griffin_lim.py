"""Fast Griffin-Lim phase retrieval on the HIP STFT kernels: the functional layer under
``padertorch_amd.contrib.mk.synthesis.parametric.griffin_lim`` (reference:
``padertorch/contrib/mk/synthesis/parametric/griffin_lim.py:32-156``).

* :func:`gl_project`     ``P = a y / |y|`` (``angle(0) := 0``), differentiable in ``a`` (the phase is a constant)
* :func:`gl_update`      lines 137-142 as one elementwise kernel on a computed ``STFT(iSTFT(P))``
* :func:`gl_iterations`  the whole loop: per iteration ``istft_kernel``, one update launch (the forward STFT with the update as its
  epilogue where a register-FFT plan exists and :data:`PATH` allows it, otherwise forward STFT + :func:`gl_update`) and the
  one-workgroup ``gl_finish_kernel`` that owns ``rmse[n]`` and the stop.  The stop is device data: no host read inside the loop, so the
  loop can be captured in a ``torch.cuda.graph``.

Everything is fp32 on the interleaved ``[rows, frames, F, 2]`` layout.
"""
import collections

import torch

from .. import _lib
from . import library
from ._stft import STFT, _geom_list

__all__ = ['gl_project', 'gl_update', 'gl_iterations', 'GriffinLimInfo', 'PATH', 'POLL_EVERY']

#: which update launch :func:`gl_iterations` uses.  ``'auto'`` selects by the FFT size: the fused epilogue where ``stft.size`` has a
#: register-FFT plan (measured faster at both benchmark shapes, profiles/griffin_lim.txt), the composed path elsewhere.  ``'fused'``
#: (raises where no plan exists) and ``'composed'`` pin a path: the tests compare the two, scripts/bench_griffin_lim.py times both
PATH = 'auto'
#: eager mode only: the host reads the ``done`` word every this many iterations and stops launching once it is set (0: never).
#: The result does not depend on it - a launch behind the stop writes nothing.
POLL_EVERY = 8

#: ``rmse`` float32 ``[iterations]`` (NaN behind the stop), ``num_iterations`` int32 scalar, ``x`` complex64 - all on the device
GriffinLimInfo = collections.namedtuple('GriffinLimInfo', ['rmse', 'num_iterations', 'x'])


class _GlProjectFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a, y):
        _lib.require_gpu(a, y)
        ctx.save_for_backward(y)
        return torch.ops.ptmi.gl_project(a, y)

    @staticmethod
    def backward(ctx, g):
        y, = ctx.saved_tensors
        return torch.ops.ptmi.gl_project_backward(g.contiguous(), y), None


def gl_project(a, y):
    """``a [...]`` float32, ``y [..., 2]`` interleaved float32 -> ``P = a y / |y|`` ``[..., 2]``.  A bin with ``y == 0`` gives ``(a, 0)``,
    one with ``a == 0`` gives 0, one with a denormal ``|y|^2`` the correct unit phasor.  ``dP/da = Re(conj(u) g)``; no gradient to ``y``."""
    return _GlProjectFn.apply(a.contiguous(), y.detach().contiguous())


def gl_update(xnew, x, a, alpha, P, partials, state):
    """See ``torch.ops.ptmi.gl_update``: ``x`` and ``P`` are updated in place."""
    _lib.require_gpu(xnew, x, a, P)
    torch.ops.ptmi.gl_update(xnew, x, a, float(alpha), P, partials, state)


def use_fused(stft, path=None):
    path = PATH if path is None else path
    assert path in ('auto', 'fused', 'composed'), path
    has_plan = stft.size in library.GL_PLAN_SIZES
    if path == 'fused' and not has_plan:
        raise RuntimeError(f'griffin_lim: the fused update needs an FFT size in {library.GL_PLAN_SIZES}, not {stft.size}')
    return has_plan and path != 'composed'


def round_trip_samples(stft: STFT, frames):
    """Samples of ``stft.inverse`` of ``frames`` frames; asserts that their STFT has ``frames`` frames again (the loop's buffers have
    one shape)."""
    samples = int(_lib.load().ptmi_istft_num_samples(stft._geom, frames))
    back = int(_lib.load().ptmi_stft_num_frames(stft._geom, samples)) if samples > 0 else 0
    assert back == frames, (
        f'griffin_lim: STFT(iSTFT(.)) does not return to {frames} frames: the inverse of {frames} frames has {samples} samples, whose '
        f'STFT has {back} frames (size {stft.size}, shift {stft.shift}, window_length {stft.window_length}, fading {stft.fading!r}, '
        f'pad {stft.pad})')
    return samples


def gl_iterations(a, x, P, stft: STFT, alpha, iterations, atol, *, path=None, poll=None):
    """``a [rows, frames, F]``, ``x`` / ``P [rows, frames, F, 2]`` float32 (updated in place) -> :class:`GriffinLimInfo` with ``x`` the
    complex view of the updated buffer."""
    _lib.require_gpu(a, x, P)
    samples = round_trip_samples(stft, a.shape[1])
    state, partials, rmse = library.gl_state(a.device, iterations)
    if poll is None:
        poll = POLL_EVERY
    if torch.cuda.is_current_stream_capturing():
        poll = 0
    tb = stft._tables.get(a.device)
    torch.ops.ptmi.gl_iterations(a, x, P, tb['syn'], tb['window'], tb['twiddle'], _geom_list(stft), samples, float(alpha),
                                 int(iterations), float(atol), use_fused(stft, path), int(poll), rmse, partials, state)
    return GriffinLimInfo(rmse, state[1], torch.view_as_complex(x))
