"""The 2-D convolution block of ``padertorch/contrib/je/modules/conv.py`` and ``Pool2d`` of ``conv_utils.py`` on the kernels of
``csrc/je_conv2d.hip``: the functional layer under ``Conv2d`` / ``CNN2d`` / ``Pool2d``.

Activations are channels-last rows ``[B F T, C]`` (row ``(b F + f) T + t``; the row stride may exceed ``C``).  Seen as ``B F`` examples
of ``T`` rows these are the rows of ``ops.je_conv``: the statistics, the norm / activation / gate / residual epilogue and its backward are
that module's kernels, unchanged, with every example's length repeated ``F`` times.

    planes(x [B, C, F, T]) -> [B F T, C]      in place when ``x`` is the permuted view of such rows (what :func:`unplanes` returns), else
                                              one gather launch (``ops.seq_pool.rows_layout``)
    unplanes(rows, B, F, T) -> [B, C, F, T]   the permuted view, no copy
    conv_block2d(...)                         one ``Conv2d`` block, forward and hand-written backward (one ``autograd.Function``):
        pre_activation    a = act(norm(x))    ``je_conv_stats`` + ``je_conv_apply`` on the input
        convolution       z, g = bias + the direct convolution of ``a`` (``je_conv2d_forward``: the input halo of a pixel tile is staged
                          once in LDS, split into fp16 hi / lo there; no padded copy, no plane of tap products); with no normalisation
                          behind it the epilogue ``act(z) sigmoid(g) + residual`` is part of that launch
        norm              ``je_conv_stats``, then ``je_conv_apply``
    pool2d(x_rows, ...)                       max (int64 indices on the padded and trimmed plane) or average pooling, with backward

The backward recomputes ``act'`` and the sigmoid from the saved ``z`` and ``g`` (``je_conv_apply_backward``); ``dx`` is the same
convolution kernel on ``dz`` (and ``dg``) with flipped taps and, for a stride, zeros inserted in LDS; ``dW`` is ``je_conv2d_wgrad`` (the
reduction over the pixels, slabs summed in order); bias gradients are ``wavenet_colsum``.  Operand scales are measured into words a
captured graph zeroes itself, so forward + backward capture in a plain ``torch.cuda.graph``.  fp32 on the GPU only; nothing is read on
the host.  A geometry whose halo does not fit the LDS of a workgroup raises ``NotImplementedError`` in the first forward; one whose weight
gradient alone does not fit (``ptmi_je_conv2d_wgrad_lds``) raises it in the forward too when a weight requires a gradient.
"""
import weakref
from collections import namedtuple

import torch
from torch.autograd.function import once_differentiable

from .. import _lib
from . import library  # noqa: F401  (registers torch.ops.ptmi)
from . import seq_pool as _seq
from .je_conv import ACTIVATIONS, _check

__all__ = ['planes', 'unplanes', 'conv_block2d', 'pool2d', 'BlockConfig2d', 'wgrad_slabs', 'invalidate']

#: B, F_in, T_in, F_out, T_out: the planes; K, stride, dilation, front: pairs (f, t); norm: None / 'batch' / 'sequence'; eps; act: code of
#: ACTIVATIONS; act_p: the negative slope / alpha; pre: pre_activation
BlockConfig2d = namedtuple('BlockConfig2d', 'B F_in T_in F_out T_out K stride dilation front norm eps act act_p pre')

#: the weight gradient's slabs: workgroups to aim for (two per compute unit) and the workspace bound in bytes
WGRAD_WORKGROUPS = 512
WGRAD_WORKSPACE_BYTES = 64 << 20


def planes(x):
    """``x [B, C, F, T]`` -> ``([B F T, C]`` with unit inner stride, ``B, F, T)``."""
    _check('je_conv2d', x)
    if x.dim() != 4 or x.numel() == 0:
        raise ValueError(f'je_conv2d: x [B, C, F, T], got {tuple(x.shape)}')
    B, C, F, T = x.shape
    sb, sc, sf, st = x.stride()
    # in place: the permuted view of rows (channel stride 1, row stride st >= C, f and b strides composing); a single pixel per example
    # has no row stride to read, so it takes the gather
    if (C == 1 or sc == 1) and st >= C and (F == 1 or sf == T * st) and (B == 1 or sb == F * T * st) and F * T > 1:
        return x.as_strided((B * F * T, C), (st, 1)), B, F, T
    if not (F == 1 or T == 1 or sf == T * st):
        x = x.contiguous()                  # f and t do not compose into one row axis (a last axis with gaps): a copy, then the gather
    r = _seq.rows_layout(x.as_strided((B, F * T, C), (x.stride(0), x.stride(3) if T > 1 else x.stride(2), x.stride(1))))
    return r.view(B * F * T, C), B, F, T


def unplanes(r, B, F, T):
    """``[B F T, C]`` contiguous -> the view ``[B, C, F, T]``."""
    return r.view(B, F, T, r.shape[1]).permute(0, 3, 1, 2)


def wgrad_slabs(B, F_out, T_out, G, C_out, C_in, taps):
    """How many ranges of pixel tiles (8 x 16 output pixels) the weight gradient is summed over: enough workgroups for the compute
    units, never more than tiles, the fp32 workspace ``slabs G C_out C_in taps`` under ``WGRAD_WORKSPACE_BYTES``; every range holds a
    tile."""
    tiles = B * -(-F_out // 8) * -(-T_out // 16)
    groups = -(-G * C_out // 64) * -(-C_in * taps // 64)
    slabs = min(tiles, -(-WGRAD_WORKGROUPS // groups), max(1, WGRAD_WORKSPACE_BYTES // (4 * G * C_out * C_in * taps)), 65535)
    per = -(-tiles // slabs)
    return -(-tiles // per)


def _word(*tensors):
    """The device word with the bits of the largest ``|value|`` of the rows ``tensors``; a captured graph zeroes it by a node of its own."""
    word = torch.zeros(1, dtype=torch.int32, device=tensors[0].device)
    for t in tensors:
        t2 = t.reshape(1, -1) if t.dim() != 2 else t
        _lib.call('ptmi_absmax_accumulate', t2.data_ptr(), t2.shape[0], t2.shape[1], max(t2.stride(0), t2.shape[1]), word.data_ptr(),
                  _lib.stream(t2.device))
    return word


# the weight planes, valid while the very weights are alive and unmodified: key -> (weak references, versions, pointers, value)
_FORMS = {}


def invalidate():
    """Drop the cached weight planes (after an in-place edit of a weight that bypasses its version counter)."""
    _FORMS.clear()


def _planes_form(weight, gate_weight, geom, input_grad):
    """``(planes, scale word)`` of the weights for the launch ``geom``, cached under ``ops.je_conv._taps_form``'s rule."""
    ps = tuple(p for p in (weight, gate_weight) if p is not None)
    key = tuple(id(p) for p in ps) + (input_grad,) + tuple(geom[11:17])
    sig = tuple((p._version, p.data_ptr()) for p in ps)
    # inside a capture the form is made anew: a graph must not hold planes that a later weight update frees or leaves stale
    capturing = torch.cuda.is_current_stream_capturing()
    hit = None if capturing else _FORMS.get(key)
    if hit is not None and hit[1] == sig and all(r() is p for r, p in zip(hit[0], ps)):
        return hit[2]
    with torch.no_grad():
        ws = [p.detach() for p in ps]
        amax = _word(*ws)
        form = (torch.ops.ptmi.je_conv2d_pack(ws[0], ws[1] if len(ws) == 2 else None, amax, geom, input_grad), amax)
    if not capturing:
        if len(_FORMS) > 1024:
            _FORMS.clear()
        _FORMS[key] = (tuple(weakref.ref(p) for p in ps), sig, form)
    return form


def _wgrad_geom(cfg, C_in, C_out, G, KF, KT):
    """The first 16 geometry values of ``ptmi_je_conv2d_wgrad``."""
    return [cfg.B, cfg.F_in, cfg.T_in, C_in, cfg.F_out, cfg.T_out, C_out, G, KF, KT, *cfg.stride, *cfg.dilation, *cfg.front]


class _Block2dFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, residual, weight, bias, gate_weight, gate_bias, gamma, beta, slope, fixed, lengths, cfg):
        ops = torch.ops.ptmi
        B, per, act, p = cfg.B, cfg.norm == 'sequence', cfg.act, cfg.act_p
        C_out, C_in, KF, KT = weight.shape
        G = 1 if gate_weight is None else 2
        has_norm = cfg.norm is not None
        a, stats = x, None
        if cfg.pre:
            if has_norm:
                stats = fixed if fixed is not None else ops.je_conv_stats(x, lengths, B * cfg.F_in, cfg.T_in, per, cfg.eps)
            if has_norm or act:
                a = ops.je_conv_apply(x, None, None, stats, gamma, beta, lengths, slope, B * cfg.F_in, cfg.T_in, per, act, p)
        geom = [B, cfg.F_in, cfg.T_in, C_in, 1, 1, 1, cfg.F_out, cfg.T_out, C_out, G, KF, KT, *cfg.stride, *cfg.dilation, *cfg.front]
        w_planes, amax_w = _planes_form(weight, gate_weight, geom, False)
        amax_a = _word(a)
        if cfg.pre or not has_norm:
            act_post = 0 if cfg.pre else act
            fused = bool(act_post) or G == 2 or residual is not None
            z, gz, out = ops.je_conv2d_forward(a, None, w_planes, amax_a, amax_w, bias, gate_bias, residual, slope, geom, act_post, p, fused)
            if not fused:
                out = z
        else:
            z, gz, _ = ops.je_conv2d_forward(a, None, w_planes, amax_a, amax_w, bias, gate_bias, None, None, geom, 0, 0., False)
            stats = fixed if fixed is not None else ops.je_conv_stats(z, lengths, B * cfg.F_out, cfg.T_out, per, cfg.eps)
            out = ops.je_conv_apply(z, gz, residual, stats, gamma, beta, lengths, slope, B * cfg.F_out, cfg.T_out, per, act, p)
        ctx.save_for_backward(x, a if a is not x else None, z, gz, stats, weight, gate_weight, gamma, beta, slope, lengths, amax_a)
        ctx.cfg, ctx.G, ctx.fixed = cfg, G, fixed is not None
        if stats is None or fixed is not None:
            return out, None
        ctx.mark_non_differentiable(stats)
        return out, stats

    @staticmethod
    @once_differentiable
    def backward(ctx, dout, _dstats):
        ops = torch.ops.ptmi
        x, a, z, gz, stats, weight, gate_weight, gamma, beta, slope, lengths, amax_a = ctx.saved_tensors
        cfg, G, need = ctx.cfg, ctx.G, ctx.needs_input_grad
        a = x if a is None else a
        B, per, act, p = cfg.B, cfg.norm == 'sequence', cfg.act, cfg.act_p
        C_out, C_in, KF, KT = weight.shape
        has_norm = cfg.norm is not None
        want = (has_norm and (need[6] or need[7])) or (act == ACTIVATIONS['prelu'] and need[8])
        dout = dout.contiguous()
        dparams = None
        BO, BI = B * cfg.F_out, B * cfg.F_in
        if cfg.pre:
            dz, dgz = dout, None
            if G == 2:
                dz, dgz, _ = ops.je_conv_apply_backward(dout, z, gz, None, None, None, None, None, BO, cfg.T_out, False, False, 0, 0., False)
        elif not has_norm and not act and G == 1:
            dz, dgz = dout, None
        else:
            dz, dgz, dparams = ops.je_conv_apply_backward(dout, z, gz, stats, gamma, beta, lengths, slope, BO, cfg.T_out, per, ctx.fixed, act,
                                                          p, want)
        db = ops.wavenet_colsum(dz) if need[3] else None
        dgb = ops.wavenet_colsum(dgz) if need[5] else None
        amax_d = _word(dz) if dgz is None else _word(dz, dgz)
        dw = dgw = None
        if need[2] or need[4]:
            slabs = wgrad_slabs(B, cfg.F_out, cfg.T_out, G, C_out, C_in, KF * KT)
            dW = ops.je_conv2d_wgrad(dz, dgz, a, amax_d, amax_a, _wgrad_geom(cfg, C_in, C_out, G, KF, KT), slabs)
            dw, dgw = dW[0], (dW[1] if G == 2 else None)
        dx = None
        pre_stage = cfg.pre and (has_norm or bool(act))
        if need[0] or (pre_stage and want):
            front = [(k - 1) * d - f for k, d, f in zip((KF, KT), cfg.dilation, cfg.front)]
            geom = [B, cfg.F_out, cfg.T_out, C_out, G, *cfg.stride, cfg.F_in, cfg.T_in, C_in, 1, KF, KT, 1, 1, *cfg.dilation, *front]
            t_planes, amax_w = _planes_form(weight, gate_weight, geom, True)
            dx = ops.je_conv2d_forward(dz, dgz, t_planes, amax_d, amax_w, None, None, None, None, geom, 0, 0., False)[0]
            if pre_stage:
                dx, _, dparams = ops.je_conv_apply_backward(dx, x, None, stats, gamma, beta, lengths, slope, BI, cfg.T_in, per, ctx.fixed, act,
                                                            p, want)
        C = gamma.numel() if gamma is not None else (beta.numel() if beta is not None else 0)
        dgamma = dparams[:C].view(gamma.shape) if dparams is not None and gamma is not None and need[6] else None
        dbeta = dparams[dparams.numel() // 2:][:C].view(beta.shape) if dparams is not None and beta is not None and need[7] else None
        dslope = dparams[-1:].view(slope.shape) if dparams is not None and slope is not None and need[8] else None
        return (dx if need[0] else None, dout if need[1] else None, dw if need[2] else None, db, dgw if need[4] else None, dgb, dgamma,
                dbeta, dslope, None, None, None)


def conv_block2d(x, cfg, weight, bias=None, gate_weight=None, gate_bias=None, gamma=None, beta=None, slope=None, fixed=None, lengths=None,
                 residual=None):
    """One block on rows: ``x [B F_in T_in, C_in]`` -> ``(out [B F_out T_out, C_out], stats [groups, 4, C] or None)``.  ``weight
    [C_out, C_in, K_f, K_t]`` and ``gate_weight`` are the ``torch.nn.Conv2d`` parameters; ``gamma`` / ``beta`` and ``lengths`` (a CUDA
    int32 / int64 vector of ``B F`` entries: every example's ``t`` length repeated ``F`` times, of the input with ``cfg.pre`` else of the
    output) belong to ``cfg.norm`` ('batch': one group over ``b, f, t``; 'sequence': one per ``(b, f)``); the rest as
    ``ops.je_conv.conv_block``."""
    _check('je_conv2d.conv_block2d', x, residual, weight, bias, gate_weight, gate_bias, gamma, beta, slope, fixed)
    if x.dim() != 2 or weight.dim() != 4 or x.shape != (cfg.B * cfg.F_in * cfg.T_in, weight.shape[1]):
        raise ValueError(f'je_conv2d.conv_block2d: x [{cfg.B * cfg.F_in * cfg.T_in}, {weight.shape[1]}], got {tuple(x.shape)}')
    if cfg.act == ACTIVATIONS['prelu'] and (slope is None or slope.numel() != 1):
        raise NotImplementedError('je_conv2d.conv_block2d: a PReLU with one parameter')
    if torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in (weight, gate_weight)):
        # a layer whose weight gradient is not built says so here, not by a status code in the first backward
        C_out, C_in, KF, KT = weight.shape
        wgeom = _wgrad_geom(cfg, C_in, C_out, 1 if gate_weight is None else 2, KF, KT)
        if _lib.load().ptmi_je_conv2d_wgrad_lds(_lib.int64s(*wgeom, C_in)) < 1:
            raise NotImplementedError('je_conv2d.conv_block2d: the weight gradient of this geometry does not fit the LDS of a workgroup '
                                      f'(the layer runs with weights that do not require a gradient): {wgeom}')
    cont = [None if t is None else t.contiguous() for t in (weight, bias, gate_weight, gate_bias)]
    flat = [None if t is None else t.reshape(-1) for t in (gamma, beta)]
    if cfg.norm is None:
        flat, fixed, lengths = [None, None], None, None
    return _Block2dFn.apply(x, residual, *cont, *flat, slope, fixed, lengths, cfg)


class _Pool2dFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, geom, max_pool):
        y, index = torch.ops.ptmi.je_pool2d_forward(x, geom, max_pool)
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
        return torch.ops.ptmi.je_pool2d_backward(dy.contiguous(), index, geom, max_pool), None, None


def pool2d(x, B, plane_in, plane_out, size, stride, front, max_pool):
    """``x [B F_in T_in, C]`` -> ``(y [B F_out T_out, C], index int64 or None)``: windows of ``size`` every ``stride`` (pairs) on the plane
    padded with ``front`` zeros (and zeros behind); the indices are ``f T_p + t`` on the padded plane trimmed to whole windows."""
    _check('je_conv2d.pool2d', x)
    geom = [B, *plane_in, *plane_out, x.shape[1], *size, *stride, *front]
    return _Pool2dFn.apply(x, [int(v) for v in geom], bool(max_pool))
