"""The convolution block of ``padertorch/contrib/je/modules/conv.py`` and the pools of ``conv_utils.py`` on the kernels of
``csrc/je_conv.hip``: the functional layer under ``padertorch_amd.contrib.je.modules.conv``.

Activations are channels-last rows ``[B T, C]`` (row ``b T + t``; the row stride may exceed ``C``), so a layer's channel products are ONE
planes GEMM over all examples.

    rows(x [B, C, T]) -> [B T, C]            in place when ``x`` is the transposed view of rows (what :func:`unrows` returns), else one
                                             gather launch (``ops.seq_pool.rows_layout``)
    unrows(rows, B, T) -> [B, C, T]          the transposed view, no copy
    conv_block(...)                          one ``Conv1d`` block, forward and hand-written backward (one ``autograd.Function``):
        pre_activation    a = act(norm(x))   ``je_conv_stats`` + ``je_conv_apply`` on the input
        GEMM              P [B T_in, G K C_out] = a W_taps^T (``ops.gemm``; ``W_taps`` stacks the ``K`` taps and, gated, the gate
                          convolution's: ``a`` is packed once; the planes of ``W_taps`` are cached per weight version)
        taps              z, g = bias + the K shifted rows of P: stride, dilation and padding are index arithmetic (``je_conv_taps``); with
                          no normalisation behind it the epilogue ``act(z) sigmoid(g) + residual`` is part of that launch
        norm              ``je_conv_stats`` (masked fp64 column sums), then ``je_conv_apply``: ``act(n) sigmoid(g) + residual``
    pool(x_rows, ...)                        max (with int64 indices into the padded axis) or average pooling, with backward

The backward recomputes ``act'`` and the sigmoid from the saved ``z`` and ``g`` (``je_conv_apply_backward``: one reduction launch for the
two masked column sums and the PReLU slope, one elementwise pass), writes ``dP`` in gather form (``je_conv_dtaps``) and runs two GEMMs,
``dx = dP W_taps`` and ``dW_taps = dP^T a``; bias gradients are ordered fp64 column sums (``wavenet_colsum``).  Every operand scale is
measured into a word that a captured graph zeroes itself (``ops.bigvgan._absmax``), so forward + backward capture in a plain
``torch.cuda.graph``.  fp32 on the GPU only; nothing is read on the host.
"""
import weakref
from collections import namedtuple

import torch
from torch.autograd.function import once_differentiable

from .. import _lib
from . import gemm as _gemm
from . import library
from . import seq_pool as _seq
from .bigvgan import _absmax

__all__ = ['rows', 'unrows', 'conv_block', 'pool', 'BlockConfig', 'ACTIVATIONS', 'invalidate']

ACTIVATIONS = library.JE_CONV_ACTIVATIONS

#: B, T_in, T_out, K, stride, dilation, front: the geometry; norm: None / 'batch' / 'sequence'; eps; act: code of ACTIVATIONS; act_p: the
#: negative slope / alpha; pre: pre_activation
BlockConfig = namedtuple('BlockConfig', 'B T_in T_out K stride dilation front norm eps act act_p pre')


def _check(name, *tensors):
    for t in tensors:
        if t is not None and t.dtype != torch.float32:
            raise NotImplementedError(f'{name}: float32 only, got {t.dtype}')
    _lib.require_gpu(*tensors)


def rows(x):
    """``x [B, C, T]`` -> ``([B T, C]`` with unit inner stride, ``B, T)``."""
    _check('je_conv', x)
    if x.dim() != 3 or x.numel() == 0:
        raise ValueError(f'je_conv: x [B, C, T], got {tuple(x.shape)}')
    B, C, T = x.shape
    xt = x.transpose(1, 2)
    if not xt.is_contiguous():
        inplace = T > 1 and (C == 1 or xt.stride(2) == 1) and xt.stride(1) >= C and (B == 1 or xt.stride(0) == T * xt.stride(1))
        if inplace:
            return xt.as_strided((B * T, C), (xt.stride(1), 1)), B, T
        xt = _seq.rows_layout(xt)
    return xt.view(B * T, C), B, T


def unrows(r, B, T):
    """``[B T, C]`` contiguous -> the view ``[B, C, T]``."""
    return r.view(B, T, r.shape[1]).transpose(1, 2)


# W_taps and its planes, valid while the very weights are alive and unmodified: key -> (weak references, versions, pointers, value)
_FORMS = {}
_TapsForm = namedtuple('_TapsForm', 'w n t')


def invalidate():
    """Drop the cached ``W_taps`` forms (after an in-place edit of a weight that bypasses its version counter)."""
    _FORMS.clear()


def _taps_form(weight, gate_weight):
    """``w [G K C_out, C_in]`` (row ``(q K + k) C_out + co``: tap ``k`` of output channel ``co`` of the convolution ``q``) and its planes as
    the right operand of ``a w^T`` (``n``) and of ``dP w`` (``t``)."""
    ps = tuple(p for p in (weight, gate_weight) if p is not None)
    key = tuple(id(p) for p in ps)
    sig = tuple((p._version, p.data_ptr()) for p in ps)
    # inside a capture the form is made anew: a graph must not hold planes that a later weight update frees or leaves stale
    capturing = torch.cuda.is_current_stream_capturing()
    hit = None if capturing else _FORMS.get(key)
    if hit is not None and hit[1] == sig and all(r() is p for r, p in zip(hit[0], ps)):
        return hit[2]
    with torch.no_grad():
        w = torch.cat([p.detach().permute(2, 0, 1).reshape(-1, p.shape[1]) for p in ps]).contiguous()
        amax = _absmax(w)
        form = _TapsForm(w, _gemm.pack_n(w, amax), _gemm.pack_t(w, amax))
    if not capturing:
        if len(_FORMS) > 1024:
            _FORMS.clear()
        _FORMS[key] = (tuple(weakref.ref(p) for p in ps), sig, form)
    return form


def _mm(x, y, **kw):
    """``x @ y`` on the planes GEMM with operand scales a captured graph can replay."""
    return _gemm.mm(x, y, amax_x=_absmax(x if x.stride(1) == 1 or x.shape[1] == 1 else x.t()),
                    amax_y=_absmax(y if y.stride(1) == 1 or y.shape[1] == 1 else y.t()), **kw)


class _BlockFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, residual, weight, bias, gate_weight, gate_bias, gamma, beta, slope, fixed, lengths, cfg):
        ops = torch.ops.ptmi
        B, per, act, p = cfg.B, cfg.norm == 'sequence', cfg.act, cfg.act_p
        C_out, C_in, K = weight.shape
        G = 1 if gate_weight is None else 2
        has_norm = cfg.norm is not None
        a, stats = x, None
        if cfg.pre:
            if has_norm:
                stats = fixed if fixed is not None else ops.je_conv_stats(x, lengths, B, cfg.T_in, per, cfg.eps)
            if has_norm or act:
                a = ops.je_conv_apply(x, None, None, stats, gamma, beta, lengths, slope, B, cfg.T_in, per, act, p)
        form = _taps_form(weight, gate_weight)
        M, N = B * cfg.T_in, G * K * C_out
        P = torch.empty((M, N), dtype=torch.float32, device=x.device)
        _gemm.mm_planes_(P, _gemm.pack_n(a, _absmax(a)), form.n, M, N, C_in)
        geom = [B, cfg.T_in, cfg.T_out, C_out, K, cfg.stride, cfg.dilation, cfg.front, G]
        if cfg.pre or not has_norm:
            act_post = 0 if cfg.pre else act
            fused = bool(act_post) or G == 2 or residual is not None
            z, gz, out = ops.je_conv_taps(P, bias, gate_bias, residual, slope, geom, act_post, p, fused)
            if not fused:
                out = z
        else:
            z, gz, _ = ops.je_conv_taps(P, bias, gate_bias, None, None, geom, 0, 0., False)
            stats = fixed if fixed is not None else ops.je_conv_stats(z, lengths, B, cfg.T_out, per, cfg.eps)
            out = ops.je_conv_apply(z, gz, residual, stats, gamma, beta, lengths, slope, B, cfg.T_out, per, act, p)
        ctx.save_for_backward(x, a if a is not x else None, z, gz, stats, weight, gate_weight, gamma, beta, slope, lengths)
        ctx.cfg, ctx.geom, ctx.fixed = cfg, geom, fixed is not None
        if stats is None or fixed is not None:
            return out, None
        ctx.mark_non_differentiable(stats)
        return out, stats

    @staticmethod
    @once_differentiable
    def backward(ctx, dout, _dstats):
        ops = torch.ops.ptmi
        x, a, z, gz, stats, weight, gate_weight, gamma, beta, slope, lengths = ctx.saved_tensors
        cfg, geom, need = ctx.cfg, ctx.geom, ctx.needs_input_grad
        a = x if a is None else a
        B, per, act, p = cfg.B, cfg.norm == 'sequence', cfg.act, cfg.act_p
        C_out, C_in, K = weight.shape
        G = geom[8]
        has_norm = cfg.norm is not None
        want = (has_norm and (need[6] or need[7])) or (act == ACTIVATIONS['prelu'] and need[8])
        dout = dout.contiguous()
        dparams = None
        if cfg.pre:
            dz, dgz = dout, None
            if G == 2:
                dz, dgz, _ = ops.je_conv_apply_backward(dout, z, gz, None, None, None, None, None, B, cfg.T_out, False, False, 0, 0., False)
        elif not has_norm and not act and G == 1:
            dz, dgz = dout, None
        else:
            dz, dgz, dparams = ops.je_conv_apply_backward(dout, z, gz, stats, gamma, beta, lengths, slope, B, cfg.T_out, per, ctx.fixed, act,
                                                          p, want)
        db = ops.wavenet_colsum(dz) if need[3] else None
        dgb = ops.wavenet_colsum(dgz) if need[5] else None
        plain = K == 1 and G == 1 and cfg.stride == 1 and cfg.front == 0 and cfg.T_in == cfg.T_out
        dP = dz if plain else ops.je_conv_dtaps(dz, dgz, geom)
        dw = dgw = None
        if need[2] or need[4]:
            dW = _mm(dP.t(), a)                                                     # [G K C_out, C_in]: the reduction runs over B T_in
            dw = dW[:K * C_out].view(K, C_out, C_in).permute(1, 2, 0)
            if G == 2:
                dgw = dW[K * C_out:].view(K, C_out, C_in).permute(1, 2, 0)
        dx = None
        pre_stage = cfg.pre and (has_norm or bool(act))
        if need[0] or (pre_stage and want):
            form = _taps_form(weight, gate_weight)
            M, N = B * cfg.T_in, G * K * C_out
            dx = torch.empty((M, C_in), dtype=torch.float32, device=dout.device)
            _gemm.mm_planes_(dx, _gemm.pack_n(dP, _absmax(dP)), form.t, M, C_in, N)
            if pre_stage:
                dx, _, dparams = ops.je_conv_apply_backward(dx, x, None, stats, gamma, beta, lengths, slope, B, cfg.T_in, per, ctx.fixed, act,
                                                            p, want)
        C = gamma.numel() if gamma is not None else (beta.numel() if beta is not None else 0)
        dgamma = dparams[:C].view(gamma.shape) if dparams is not None and gamma is not None and need[6] else None
        dbeta = dparams[dparams.numel() // 2:][:C].view(beta.shape) if dparams is not None and beta is not None and need[7] else None
        dslope = dparams[-1:].view(slope.shape) if dparams is not None and slope is not None and need[8] else None
        return (dx if need[0] else None, dout if need[1] else None, dw if need[2] else None, db, dgw if need[4] else None, dgb, dgamma,
                dbeta, dslope, None, None, None)


def conv_block(x, cfg, weight, bias=None, gate_weight=None, gate_bias=None, gamma=None, beta=None, slope=None, fixed=None, lengths=None,
               residual=None):
    """One block on rows: ``x [B T_in, C_in]`` -> ``(out [B T_out, C_out], stats [groups, 4, C] or None)``.  ``weight [C_out, C_in, K]`` and
    ``gate_weight`` are the ``torch.nn.Conv1d`` parameters; ``gamma`` / ``beta`` (any shape with ``C`` elements) and ``lengths`` (a CUDA
    int32 / int64 vector, of the input with ``cfg.pre`` else of the output) belong to ``cfg.norm``; ``fixed [1, 4, C]`` (mean, rstd, -, -)
    replaces the measured statistics; ``slope``: the PReLU's parameter; ``residual [B T_out, C_out]`` is added behind the activation."""
    _check('je_conv.conv_block', x, residual, weight, bias, gate_weight, gate_bias, gamma, beta, slope, fixed)
    if x.dim() != 2 or weight.dim() != 3 or x.shape != (cfg.B * cfg.T_in, weight.shape[1]):
        raise ValueError(f'je_conv.conv_block: x [{cfg.B * cfg.T_in}, {weight.shape[1]}], got {tuple(x.shape)}')
    if cfg.act == ACTIVATIONS['prelu'] and (slope is None or slope.numel() != 1):
        raise NotImplementedError('je_conv.conv_block: a PReLU with one parameter')
    cont = [None if t is None else t.contiguous() for t in (weight, bias, gate_weight, gate_bias)]
    flat = [None if t is None else t.reshape(-1) for t in (gamma, beta)]
    if cfg.norm is None:
        flat, fixed, lengths = [None, None], None, None
    return _BlockFn.apply(x, residual, *cont, *flat, slope, fixed, lengths, cfg)


class _NormActFn(torch.autograd.Function):
    """``act(norm(x))`` alone: the ``input_norm`` / ``output_norm`` of a ``CNN1d``."""

    @staticmethod
    def forward(ctx, x, gamma, beta, slope, fixed, lengths, B, T, norm, eps, act, p):
        ops = torch.ops.ptmi
        per = norm == 'sequence'
        stats = fixed if fixed is not None else ops.je_conv_stats(x, lengths, B, T, per, eps)
        out = ops.je_conv_apply(x, None, None, stats, gamma, beta, lengths, slope, B, T, per, act, p)
        ctx.save_for_backward(x, gamma, beta, slope, stats, lengths)
        ctx.cfg = (B, T, per, fixed is not None, act, p)
        if fixed is not None:
            return out, None
        ctx.mark_non_differentiable(stats)
        return out, stats

    @staticmethod
    @once_differentiable
    def backward(ctx, dout, _):
        x, gamma, beta, slope, stats, lengths = ctx.saved_tensors
        B, T, per, fixed, act, p = ctx.cfg
        need = ctx.needs_input_grad
        want = need[1] or need[2] or (act == ACTIVATIONS['prelu'] and need[3])
        dx, _, dparams = torch.ops.ptmi.je_conv_apply_backward(dout.contiguous(), x, None, stats, gamma, beta, lengths, slope, B, T, per,
                                                               fixed, act, p, want)
        C = x.shape[1]
        return (dx if need[0] else None, dparams[:C] if need[1] else None, dparams[C:2 * C] if need[2] else None,
                dparams[-1:].view(slope.shape) if slope is not None and need[3] else None, None, None, None, None, None, None, None, None)


def norm_act(x, B, T, norm, eps, act, act_p, gamma=None, beta=None, slope=None, fixed=None, lengths=None):
    """``x [B T, C]`` -> ``(act(norm(x)), stats or None)`` with the masked statistics of ``norm`` ('batch' / 'sequence') or ``fixed``."""
    _check('je_conv.norm_act', x, gamma, beta, slope, fixed)
    flat = [None if t is None else t.reshape(-1) for t in (gamma, beta)]
    return _NormActFn.apply(x, *flat, slope, fixed, lengths, B, T, norm, eps, act, act_p)


class _AddFn(torch.autograd.Function):
    """``a + b`` on rows (a second residual connection that ends at the same layer): ``je_conv_apply`` with nothing but the residual."""

    @staticmethod
    def forward(ctx, a, b, B, T):
        return torch.ops.ptmi.je_conv_apply(a, None, b, None, None, None, None, None, B, T, False, 0, 0.)

    @staticmethod
    def backward(ctx, g):
        return g, g, None, None


def add(a, b, B, T):
    _check('je_conv.add', a, b)
    return _AddFn.apply(a, b, B, T)


class _PoolFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, geom, max_pool):
        y, index = torch.ops.ptmi.je_pool_forward(x, geom, max_pool)
        ctx.save_for_backward(index)
        ctx.cfg = (geom, max_pool)
        if max_pool:
            ctx.mark_non_differentiable(index)
        return y, index

    @staticmethod
    @once_differentiable
    def backward(ctx, dy, _):
        index, = ctx.saved_tensors
        geom, max_pool = ctx.cfg
        return torch.ops.ptmi.je_pool_backward(dy.contiguous(), index, geom, max_pool), None, None


def pool(x, B, T_in, T_out, size, stride, front, max_pool):
    """``x [B T_in, C]`` -> ``(y [B T_out, C], index int64 or None)``: windows of ``size`` every ``stride`` on the axis padded with ``front``
    zeros (and zeros behind); the indices count on the padded axis."""
    _check('je_conv.pool', x)
    return _PoolFn.apply(x, [B, T_in, T_out, x.shape[1], int(size), int(stride), int(front)], bool(max_pool))
