"""The convolutions of the BigVGAN generator on HIP kernels (``csrc/bigvgan.hip``), inference only: the functional layer under
``padertorch_amd.contrib.mk.synthesis.vocoder.nvidia_bigvgan.bigvgan`` (reference: ``nvidia_bigvgan/bigvgan.py``).

* :func:`conv1d`            a dilated ``Conv1d`` with "same" zero padding, on one of two paths behind one epilogue
                            ``v = scale (conv + bias + residual)``, ``out = v`` or ``out += v``:
                            ``'gemm'``    ``P_b [K C_out, T] = Wtaps [K C_out, C_in] x_b [C_in, T]`` on the split-fp16 planes GEMM
                            (``ops.gemm``; ``x_b`` is packed where it lies, ``Wtaps`` once per weight), then ``bigvgan_taps`` adds the ``K``
                            shifted rows; ``'direct'``  ``bigvgan_conv_direct``: fp32 FMAs out of LDS, no ``P`` (narrow layers)
* :func:`conv_transpose1d`  ``ConvTranspose1d(C_in, C_out, k, stride, padding=(k - stride) // 2)``: a GEMM and the gather-form overlap-add
* :func:`conv_post`         ``C -> 1`` channel, then ``tanh`` or the clamp to [-1, 1], one launch
* :func:`fold_weight_norm`  ``g v / |v|`` as ``torch.nn.utils.weight_norm`` defines it

fp32, ``[B, C, T]``.  None of them is differentiable, nothing is read on the host, every sum has one fixed order: the same input gives the
same bits, eagerly and in a replayed ``torch.cuda.graph``.
"""
import weakref

import torch

from .. import _lib
from . import gemm
from . import library  # noqa: F401  (registers torch.ops.ptmi.bigvgan_*)

__all__ = ['conv1d', 'conv_transpose1d', 'conv_post', 'fold_weight_norm', 'choose_path', 'direct_ok', 'invalidate', 'DIRECT_MAX_CHANNELS',
           'DIRECT_MAX_TAPS', 'DIRECT_MAX_HALO', 'DIRECT_TILE', 'TAPS_TILE', 'MAX_STRIDE', 'DIRECT_UP_TO']

#: the limits of ``bigvgan_conv_direct`` (``ptmi_bigvgan_direct_ok``): input channels, taps, ``(K - 1) dilation / 2``
DIRECT_MAX_CHANNELS = 128
DIRECT_MAX_TAPS = 11
DIRECT_MAX_HALO = 64
#: samples of a row per workgroup (``ptmi_bigvgan_tile``)
DIRECT_TILE = 512
TAPS_TILE = 1024
#: the largest stride of :func:`conv_transpose1d`
MAX_STRIDE = 8
#: the automatic choice: taps ``K`` -> the widest ``C_in`` that still runs on the direct path (0: never; above it the GEMM path).  Derived
#: by ``scripts/bench_bigvgan.py`` from its table of every convolution on both paths (``profiles/bigvgan.txt``, line ``DIRECT_UP_TO``):
#: the direct kernel was faster at 24 and 32 channels (24 only at 11 taps) and slower from 48 channels on, at 100 and at 400 mel frames.
DIRECT_UP_TO = {1: 32, 3: 32, 5: 32, 7: 32, 9: 24, 11: 24}


def direct_ok(c_in, kernel_size, dilation):
    """The direct kernel covers this layer."""
    return (1 <= c_in <= DIRECT_MAX_CHANNELS and kernel_size % 2 == 1 and kernel_size <= DIRECT_MAX_TAPS
            and (kernel_size - 1) // 2 * dilation <= DIRECT_MAX_HALO)


def choose_path(c_in, kernel_size, dilation):
    """``'direct'`` or ``'gemm'`` for ``path=None``."""
    if direct_ok(c_in, kernel_size, dilation) and c_in <= DIRECT_UP_TO.get(kernel_size, 0):
        return 'direct'
    return 'gemm'


def _inference_only(what, *tensors):
    if torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in tensors):
        raise RuntimeError(f'{what}: inference only - the BigVGAN convolutions have no backward; call it under torch.no_grad() / '
                           f'torch.inference_mode() or detach the inputs')


def _check(what, x, weight, *others):
    for t in (x, weight) + others:
        if t is not None and t.dtype != torch.float32:
            raise TypeError(f'{what}: float32 only, got {t.dtype}')
    if x.dim() != 3:
        raise ValueError(f'{what}: expected x [B, C, T], got {tuple(x.shape)}')
    if weight.dim() != 3:
        raise ValueError(f'{what}: expected a weight of three axes, got {tuple(weight.shape)}')
    _inference_only(what, x, weight, *others)


# weight-derived operands, valid while the very tensor is alive and unmodified (as ops.gemm's caches; a generator has more weights than
# those hold): key -> (weak reference, version, storage pointer, value)
_FORMS = {}


def invalidate():
    """Drop the cached ``Wtaps`` planes (after an in-place edit of a weight that bypasses its version counter)."""
    _FORMS.clear()


def _weight_form(kind, p, make):
    key = (kind, id(p))
    version = None if p.is_inference() else p._version       # (a tensor made under inference_mode has no version counter: not cached)
    hit = _FORMS.get(key)
    if hit is not None and version is not None and hit[0]() is p and hit[1] == version and hit[2] == p.data_ptr():
        return hit[3]
    with torch.no_grad():
        value = make()
    # (made inside a capture it lives in the graph's pool: not for eager calls)
    if version is not None and not torch.cuda.is_current_stream_capturing():
        if len(_FORMS) > 4096:
            _FORMS.clear()
        _FORMS[key] = (weakref.ref(p), version, p.data_ptr(), value)
    return value


def _planes_of(matrix):
    """fp16 (hi, lo) planes and the scale word of a contiguous ``[rows, k]`` weight matrix."""
    return gemm.pack_n(matrix, _absmax(matrix))


def _absmax(x2d):
    """The device word with the bits of ``max |x2d|``.  Inside a ``torch.cuda.graph`` capture the word is zero-filled by a node of the
    graph (the eager pool's words are zeroed once, when their block is made: a replay would start from the last replay's maximum)."""
    if not torch.cuda.is_current_stream_capturing():
        return gemm.absmax(x2d)
    word = torch.zeros(1, dtype=torch.int32, device=x2d.device)
    _lib.call('ptmi_absmax_accumulate', x2d.data_ptr(), x2d.shape[0], x2d.shape[1], max(x2d.stride(0), x2d.shape[1]), word.data_ptr(),
              _lib.stream(x2d.device))
    return word


def _channel_gemm(w_planes, x, rows):
    """``[B, rows, T]``: per batch entry ``W [rows, C_in] x_b [C_in, T]``; ``x_b`` goes through the pack pass for "reduction axis
    outermost" where it lies, one scale word for the whole batch."""
    B, C_in, T = x.shape
    out = torch.empty((B, rows, T), dtype=torch.float32, device=x.device)
    amax = _absmax(x.view(B * C_in, T))
    for b in range(B):
        gemm.mm_planes_(out[b], w_planes, gemm.pack_t(x[b], amax), rows, T, C_in)
    return out


def conv1d(x, weight, bias=None, dilation=1, *, residual=None, out=None, accumulate=False, scale=1.0, path=None):
    """``x [B, C_in, T]``, ``weight [C_out, C_in, K]`` (``K`` odd) -> ``[B, C_out, T]``: ``Conv1d(dilation=dilation,
    padding=(K - 1) dilation // 2)`` with the epilogue ``v = scale (conv + bias + residual)``; ``out = v``, or ``out += v`` with
    ``accumulate`` (``out`` is made when ``None``).  ``path``: ``None`` (:func:`choose_path`), ``'gemm'`` or ``'direct'``."""
    _check('bigvgan.conv1d', x, weight, bias, residual, out)
    B, C_in, T = x.shape
    C_out, wc, K = weight.shape
    dilation = int(dilation)
    if wc != C_in:
        raise ValueError(f'bigvgan.conv1d: a weight for {wc} input channels, x has {C_in}')
    if K % 2 == 0:
        raise ValueError(f'bigvgan.conv1d: an even kernel size ({K}) has no "same" padding')
    if dilation < 1:
        raise ValueError(f'bigvgan.conv1d: dilation {dilation}')
    if bias is not None and tuple(bias.shape) != (C_out,):
        raise ValueError(f'bigvgan.conv1d: a bias of shape {tuple(bias.shape)} for {C_out} output channels')
    for name, t in (('residual', residual), ('out', out)):
        if t is not None and tuple(t.shape) != (B, C_out, T):
            raise ValueError(f'bigvgan.conv1d: {name} of shape {tuple(t.shape)}, the output is {(B, C_out, T)}')
    if accumulate and out is None:
        raise ValueError('bigvgan.conv1d: accumulate=True needs out')
    if path not in (None, 'gemm', 'direct'):
        raise ValueError(f"bigvgan.conv1d: path {path!r} is not None, 'gemm' or 'direct'")
    if path == 'direct' and not direct_ok(C_in, K, dilation):
        raise ValueError(f'bigvgan.conv1d: the direct kernel covers C_in <= {DIRECT_MAX_CHANNELS}, K <= {DIRECT_MAX_TAPS} and '
                         f'(K - 1) dilation / 2 <= {DIRECT_MAX_HALO}; got C_in = {C_in}, K = {K}, dilation = {dilation}')
    if path is None:
        path = choose_path(C_in, K, dilation)
    _lib.require_gpu(x, weight, bias, residual, out)
    x = x.contiguous()
    if out is None:
        out = torch.empty((B, C_out, T), dtype=torch.float32, device=x.device)
    elif not out.is_contiguous():
        raise ValueError('bigvgan.conv1d: out must be contiguous')
    if residual is not None:
        residual = residual.contiguous()
    if out.numel() == 0:
        return out
    if path == 'direct':
        torch.ops.ptmi.bigvgan_conv_direct_(out, x, weight.detach().contiguous(), bias, residual, dilation, float(scale), bool(accumulate))
        return out
    # row k C_out + co of Wtaps: tap k of output channel co
    planes = _weight_form('taps', weight, lambda: _planes_of(weight.detach().permute(2, 0, 1).reshape(K * C_out, C_in).contiguous()))
    P = _channel_gemm(planes, x, K * C_out)
    torch.ops.ptmi.bigvgan_taps_(out, P, bias, residual, K, dilation, float(scale), bool(accumulate))
    return out


def conv_transpose1d(x, weight, bias, stride):
    """``x [B, C_in, T]``, ``weight [C_in, C_out, k]`` -> ``[B, C_out, (T - 1) stride - 2 ((k - stride) // 2) + k]``:
    ``ConvTranspose1d(stride=stride, padding=(k - stride) // 2)`` as ``G_b [C_out k, T] = W^T x_b`` and ``bigvgan_ola``."""
    _check('bigvgan.conv_transpose1d', x, weight, bias)
    B, C_in, T = x.shape
    wc, C_out, k = weight.shape
    stride = int(stride)
    if wc != C_in:
        raise ValueError(f'bigvgan.conv_transpose1d: a weight for {wc} input channels, x has {C_in}')
    if not 1 <= stride <= MAX_STRIDE:
        raise ValueError(f'bigvgan.conv_transpose1d: stride {stride} is outside 1..{MAX_STRIDE}')
    if k < stride:
        raise ValueError(f'bigvgan.conv_transpose1d: a kernel of {k} taps is shorter than the stride {stride}')
    if bias is not None and tuple(bias.shape) != (C_out,):
        raise ValueError(f'bigvgan.conv_transpose1d: a bias of shape {tuple(bias.shape)} for {C_out} output channels')
    if T == 0:
        raise ValueError('bigvgan.conv_transpose1d: an empty signal')
    _lib.require_gpu(x, weight, bias)
    x = x.contiguous()
    planes = _weight_form('ola', weight, lambda: _planes_of(weight.detach().reshape(C_in, C_out * k).t().contiguous()))
    G = _channel_gemm(planes, x, C_out * k)
    return torch.ops.ptmi.bigvgan_ola(G, bias, k, stride)


def conv_post(x, weight, bias=None, tanh=True):
    """``x [B, C, T]``, ``weight [1, C, K]`` (``K`` odd, at most 11), ``bias [1]`` or ``None`` -> ``[B, 1, T]``: the convolution, then
    ``tanh`` or (``tanh=False``) the clamp to [-1, 1], one launch; NaN stays NaN."""
    _check('bigvgan.conv_post', x, weight, bias)
    C, K = x.shape[1], weight.shape[2]
    if tuple(weight.shape[:2]) != (1, C):
        raise ValueError(f'bigvgan.conv_post: expected a weight [1, {C}, K], got {tuple(weight.shape)}')
    if K % 2 == 0 or K > DIRECT_MAX_TAPS:
        raise ValueError(f'bigvgan.conv_post: kernel size {K} is not an odd number up to {DIRECT_MAX_TAPS}')
    if bias is not None and bias.numel() != 1:
        raise ValueError(f'bigvgan.conv_post: a bias of shape {tuple(bias.shape)} for one output channel')
    _lib.require_gpu(x, weight, bias)
    return torch.ops.ptmi.bigvgan_post(x.contiguous(), weight.detach().contiguous(), None if bias is None else bias.detach().contiguous(),
                                       bool(tanh))


def fold_weight_norm(g, v):
    """``g v / |v|`` with the norm over every axis but 0: what ``torch.nn.utils.weight_norm`` (``dim=0``) computes, for ``Conv1d``
    (axis 0: output channels) and ``ConvTranspose1d`` (axis 0: input channels) alike."""
    if g.dim() != v.dim() or g.shape[0] != v.shape[0] or g.numel() != v.shape[0]:
        raise ValueError(f'fold_weight_norm: g {tuple(g.shape)} does not go with v {tuple(v.shape)}')
    norm = torch.linalg.vector_norm(v, 2, dim=tuple(range(1, v.dim())), keepdim=True)
    return v * (g / norm)
