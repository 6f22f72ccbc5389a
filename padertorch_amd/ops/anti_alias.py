"""BigVGAN's anti-aliased periodic activation on one fused HIP kernel: the functional layer under
``padertorch_amd.contrib.mk.synthesis.vocoder.nvidia_bigvgan`` (reference: ``alias_free_activation/torch/{filter,resample,act}.py`` and
``activations.py`` there).

* :func:`kaiser_sinc_filter1d`   the Kaiser-windowed sinc low-pass, designed in fp64 on the host, stored as fp32 ``[1, 1, k]``
* :func:`anti_alias_activation`  up-sampling -> Snake / SnakeBeta -> low-pass and decimation: ONE launch, the up-sampled signal stays on chip
* :func:`upsample1d`, :func:`lowpass1d`, :func:`snake`   the same kernel with the other stages switched off

All of them are differentiable in ``x`` and (where present) ``alpha`` / ``beta``; the backward is one launch that recomputes the
up-sampled signal from ``x`` (nothing but the inputs is saved) plus, when a parameter requires a gradient, the one-workgroup-per-channel
finishing kernel that adds the fp64 partials in a fixed order.  fp32, ``[B, C, T]``, replicate padding only.
"""
import math

import numpy as np
import torch

from .. import _lib
from . import library  # noqa: F401  (registers torch.ops.ptmi.anti_alias_*)

__all__ = ['kaiser_sinc_filter1d', 'anti_alias_activation', 'upsample1d', 'lowpass1d', 'snake', 'TILE', 'TILE_GENERIC', 'MAX_TAPS',
           'MAX_RATIO', 'check_stage', 'default_kernel_size']

#: outputs (forward) / input samples (backward) one workgroup owns at the default hyper-parameters (ratios 2 / 2, 12 / 12 taps) - the
#: compile-time specialisation; ``ptmi_anti_alias_tile(1)``
TILE = 1024
#: the same for every other combination; ``ptmi_anti_alias_tile(0)``
TILE_GENERIC = 256
#: the bounds of the run-time path: taps per filter and ratio per stage (``ValueError`` beyond)
MAX_TAPS = 64
MAX_RATIO = 8


def default_kernel_size(ratio):
    return int(6 * ratio // 2) * 2


def kaiser_sinc_filter1d(cutoff, half_width, kernel_size):
    """The low-pass of filter.py:30-62 as float32 ``[1, 1, kernel_size]``: ``2 cutoff * kaiser * sinc(2 cutoff * time)`` normalised to sum
    1, computed in float64 and rounded once (``cutoff == 0``: zeros)."""
    kernel_size = int(kernel_size)
    half = kernel_size // 2
    A = 2.285 * (half - 1) * math.pi * (4 * half_width) + 7.95
    if A > 50.0:
        beta = 0.1102 * (A - 8.7)
    elif A >= 21.0:
        beta = 0.5842 * (A - 21.0) ** 0.4 + 0.07886 * (A - 21.0)
    else:
        beta = 0.0
    window = np.kaiser(kernel_size, beta)                        # symmetric
    time = np.arange(-half, half) + 0.5 if kernel_size % 2 == 0 else np.arange(kernel_size, dtype=np.float64) - half
    if cutoff == 0:
        taps = np.zeros(kernel_size)
    else:
        taps = 2 * cutoff * window * np.sinc(2 * cutoff * time)
        taps = taps / taps.sum()
    return torch.from_numpy(taps.astype(np.float32)).view(1, 1, kernel_size)


def check_stage(ratio, kernel_size, up):
    """The bounds of the kernel's run-time path (``ValueError`` beyond them)."""
    what = 'up' if up else 'down'
    if not (isinstance(ratio, int) and 1 <= ratio <= MAX_RATIO):
        raise ValueError(f'anti_alias: {what}-sampling ratio {ratio!r} is outside 1..{MAX_RATIO}')
    if not (isinstance(kernel_size, int) and 1 <= kernel_size <= MAX_TAPS):
        raise ValueError(f'anti_alias: {what}-sampling kernel size {kernel_size!r} is outside 1..{MAX_TAPS}')
    if up and kernel_size < ratio:
        raise ValueError(f'anti_alias: an up-sampling filter of {kernel_size} taps is shorter than the ratio {ratio}')


def _taps(f, x, ratio, up):
    """A filter buffer (``[1, 1, k]`` or ``[k]``) as the kernel's operand: fp32, flat, on the device of ``x``."""
    if f is None:
        return None
    check_stage(int(ratio), int(f.numel()), up)
    return f.detach().reshape(-1).to(device=x.device, dtype=torch.float32).contiguous()


class _AntiAliasFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, alpha, beta, up_filter, down_filter, up_ratio, down_ratio, padding, logscale):
        ctx.shared = alpha is not None and beta is None                      # Snake: beta IS alpha
        ctx.cfg = (up_ratio, down_ratio, padding, logscale)
        a = None if alpha is None else alpha.contiguous()
        b = a if ctx.shared else (None if beta is None else beta.contiguous())
        ctx.save_for_backward(x, a, None if ctx.shared else b, up_filter, down_filter)
        return torch.ops.ptmi.anti_alias_forward(x, up_filter, down_filter, a, b, *ctx.cfg)

    @staticmethod
    def backward(ctx, g):
        x, a, b, up_filter, down_filter = ctx.saved_tensors
        if ctx.shared:
            b = a
        want = a is not None and (ctx.needs_input_grad[1] or ctx.needs_input_grad[2])
        mode = 0 if not want else (1 if ctx.shared else 2)
        dx, da, db = torch.ops.ptmi.anti_alias_backward(g.contiguous(), x, up_filter, down_filter, a, b, *ctx.cfg, mode)
        return (dx, da if mode >= 1 else None, db if mode == 2 else None, None, None, None, None, None, None)


def _apply(x, alpha, beta, up_filter, up_ratio, down_filter, down_ratio, padding, logscale):
    if x.dtype != torch.float32 or any(p is not None and p.dtype != torch.float32 for p in (alpha, beta)):
        raise TypeError(f'anti_alias: float32 only, got {x.dtype}'
                        + ''.join(f', {p.dtype}' for p in (alpha, beta) if p is not None))
    if x.dim() != 3:
        raise ValueError(f'anti_alias: expected [B, C, T], got {tuple(x.shape)}')
    for p in (alpha, beta):
        if p is not None and tuple(p.shape) != (x.shape[1],):
            raise ValueError(f'anti_alias: a parameter of shape {tuple(p.shape)} for {x.shape[1]} channels')
    for f, ratio, is_up in ((up_filter, up_ratio, True), (down_filter, down_ratio, False)):
        if f is not None:
            check_stage(int(ratio), int(f.numel()), is_up)
    _lib.require_gpu(x, alpha, beta)
    up = _taps(up_filter, x, up_ratio, True)
    down = _taps(down_filter, x, down_ratio, False)
    return _AntiAliasFn.apply(x.contiguous(), alpha, beta, up, down, int(up_ratio) if up is not None else 1,
                              int(down_ratio) if down is not None else 1, bool(padding), bool(logscale))


def anti_alias_activation(x, alpha, beta=None, *, up_filter, down_filter, up_ratio=2, down_ratio=2, alpha_logscale=False):
    """``DownSample1d(SnakeBeta(UpSample1d(x)))`` in one launch.  ``x [B, C, T]``, ``alpha`` / ``beta [C]`` (``beta=None``: Snake, whose
    magnitude parameter is ``alpha`` itself), the filters as :func:`kaiser_sinc_filter1d` returns them -> ``[B, C, ceil(up_ratio T /
    down_ratio)]``."""
    return _apply(x, alpha, beta, up_filter, up_ratio, down_filter, down_ratio, True, alpha_logscale)


def upsample1d(x, filter, ratio=2):
    """``UpSample1d``: replicate-padded transposed convolution of stride ``ratio``, times ``ratio`` -> ``[B, C, ratio T]``."""
    return _apply(x, None, None, filter, ratio, None, 1, True, False)


def lowpass1d(x, filter, stride=1, padding=True):
    """``LowPassFilter1d`` / ``DownSample1d``: (replicate-padded) FIR of stride ``stride``."""
    return _apply(x, None, None, None, 1, filter, stride, padding, False)


def snake(x, alpha, beta=None, alpha_logscale=False):
    """``x + sin^2(alpha' x) / (beta' + 1e-9)`` per channel (``beta=None``: ``beta = alpha``)."""
    return _apply(x, alpha, beta, None, 1, None, 1, True, alpha_logscale)
