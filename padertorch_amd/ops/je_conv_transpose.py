"""The transposed convolution block of ``padertorch/contrib/je/modules/conv.py`` and ``Unpool1d`` / ``Unpool2d`` of ``conv_utils.py`` on
the kernels of ``csrc/je_conv_transpose.hip``: the functional layer under ``ConvTranspose1d`` / ``ConvTranspose2d`` / ``CNNTranspose*`` /
``Unpool*``.  Rows, statistics, epilogue and operand scales are those of ``ops.je_conv2d``; the 1-D classes are planes with ``F = 1``.

    phase_table(K, stride, dilation, front)   one axis of the sub-pixel split (pure host code): for every phase ``r`` the taps ``k``
                                              that reach it and their input offsets
    plan(cfg, C_in, C_out, G)                 the launch geometry of a block (pure host code)
    conv_transpose_block(...)                 one block, forward and hand-written backward (one ``autograd.Function``):
        pre_activation    a = act(norm(x))    ``je_conv_stats`` + ``je_conv_apply`` on the input
        convolution       z, g = bias + the phase-split transposed convolution of ``a`` (``je_conv_transpose_forward``); with no
                          normalisation behind it the launch writes the trimmed window and ``act(z) sigmoid(g) + residual`` with it
        norm              the reference normalises the UNTRIMMED output with the TRIMMED lengths and trims afterwards: with a
                          normalisation behind the convolution the launch writes the untrimmed plane (``cfg.front = 0``),
                          ``je_conv_stats`` / ``je_conv_apply`` run on it and the caller trims (a view)
    unpool(x_rows, index, geom)               max unpooling by indices, or nearest upsampling without, with backward

The backward has no arithmetic kernel of its own: ``dx`` of a transposed convolution is the plain strided convolution of ``dz`` with the
same, unflipped weights (``W[C_in, C_out, K_f, K_t]`` read as a ``Conv2d`` weight), ``je_conv2d_forward`` in mode 0, a gated block's second
convolution added through that launch's residual operand; ``dW`` is ``je_conv2d_wgrad`` with the roles exchanged (``a`` on the pixel grid,
``dz`` under the taps), once per convolution (in groups of output channels where ``ptmi_je_conv2d_wgrad_lds`` refuses the whole width);
bias gradients are ``wavenet_colsum``.  A geometry the planner does not take, and a trained layer whose weight gradient does not fit
even for one output channel, raise ``NotImplementedError`` in the forward.
"""
import weakref
from collections import namedtuple
from functools import lru_cache

import torch
from torch.autograd.function import once_differentiable

from .. import _lib
from . import library  # noqa: F401  (registers torch.ops.ptmi)
from .je_conv import ACTIVATIONS, _check
from .je_conv2d import _word, wgrad_slabs

__all__ = ['phase_table', 'plan', 'conv_transpose_block', 'unpool', 'TransposeConfig', 'invalidate']

#: B, F_in, T_in: the input plane; F_out, T_out: the plane the block writes, which starts ``front`` positions into the full output (the
#: trimmed window, or with ``front = (0, 0)`` the untrimmed plane); K, stride, dilation, front: pairs (f, t); the rest as BlockConfig2d
TransposeConfig = namedtuple('TransposeConfig', 'B F_in T_in F_out T_out K stride dilation front norm eps act act_p pre')

MAX_TAPS, MAX_STRIDE, MAX_PHASES = 16, 16, 64


def phase_table(K, stride, dilation, front=0):
    """One axis of the phase split: ``[(r, [(k, offset), ...]) for r in range(stride)]``.  The output position ``o`` of the window that
    starts ``front`` positions into the full output has ``u = o + front = r + stride q``; the taps with ``k dilation = r (mod stride)``
    reach it, each from the input position ``q - offset`` with ``offset = (k dilation - r) / stride``."""
    return [(r, [(k, (k * dilation - r) // stride) for k in range(K) if (k * dilation - r) % stride == 0]) for r in range(stride)]


def plan(cfg, C_in, C_out, G):
    """The geometry list of ``torch.ops.ptmi.je_conv_transpose_*`` for a block: 16 values, then per axis the taps in phase order."""
    if max(cfg.K) > MAX_TAPS or max(cfg.stride) > MAX_STRIDE or cfg.stride[0] * cfg.stride[1] > MAX_PHASES:
        raise NotImplementedError(f'je_conv_transpose: at most {MAX_TAPS} taps and a stride of {MAX_STRIDE} per axis and {MAX_PHASES} '
                                  f'phases, got kernel {cfg.K}, stride {cfg.stride}')
    order = [k for K, s, d in zip(cfg.K, cfg.stride, cfg.dilation) for _, taps in phase_table(K, s, d) for k, _ in taps]
    return [cfg.B, cfg.F_in, cfg.T_in, C_in, cfg.F_out, cfg.T_out, C_out, G, *cfg.K, *cfg.stride, *cfg.dilation, *cfg.front, *order]


def ksteps(geom):
    """Matrix-instruction k steps per output pixel and 16 output channels, summed over the phases (``ptmi_je_conv_transpose_ksteps``)."""
    return _lib.load().ptmi_je_conv_transpose_ksteps(_lib.int64s(*geom[:16], geom[3], geom[6], *geom[16:]))


# the weight planes, valid while the very weights are alive and unmodified (ops.je_conv2d._planes_form's rule)
_FORMS = {}


def invalidate():
    _FORMS.clear()


def _cached_form(weights, key, pack):
    """``(pack(weights, amax word), amax word)``, cached under ``ops.je_conv2d._planes_form``'s rule.  A ConvTranspose1d hands in the
    ``[C_in, C_out, 1, K]`` view of its parameter: the parameter is what lives and carries the version, so the entry is keyed on it, and
    the view's own shape and address are part of the signature (two views of one tensor do not share planes)."""
    bases = tuple(p if p._base is None else p._base for p in weights)
    key = tuple(id(p) for p in bases) + key
    sig = tuple((b._version, p.data_ptr(), tuple(p.shape)) for b, p in zip(bases, weights))
    # inside a capture the form is made anew: a graph must not hold planes that a later weight update frees or leaves stale
    capturing = torch.cuda.is_current_stream_capturing()
    hit = None if capturing else _FORMS.get(key)
    if hit is not None and hit[1] == sig and all(r() is p for r, p in zip(hit[0], bases)):
        return hit[2]
    with torch.no_grad():
        ws = [p.detach() for p in weights]
        amax = _word(*ws)
        form = (pack(ws, amax), amax)
    if not capturing:
        if len(_FORMS) > 1024:
            _FORMS.clear()
        _FORMS[key] = (tuple(weakref.ref(p) for p in bases), sig, form)
    return form


def _planes_form(weight, gate_weight, geom):
    """The phase planes of a block's weights for the launch ``geom``."""
    ws = tuple(p for p in (weight, gate_weight) if p is not None)
    # the planes depend on the taps, strides and dilations and on the channel chunk, which follows the pixel tile (one grid row or more)
    one_row = (geom[4] - 1 + geom[14]) // geom[10] == geom[14] // geom[10]
    return _cached_form(ws, ('forward', *geom[8:14], one_row),
                        lambda w, amax: torch.ops.ptmi.je_conv_transpose_pack(w[0], w[1] if len(w) == 2 else None, amax, geom))


def _dx_planes_form(weight, geom):
    """``je_conv2d_forward``'s mode-0 planes of one weight read as a ``Conv2d`` weight, for the input gradient's launch ``geom``; kept
    here, on the parameter, because ``ops.je_conv2d``'s own cache is keyed on the tensor it is handed (a 1-D block's throw-away view)."""
    return _cached_form((weight,), ('dx', *geom[11:17]), lambda w, amax: torch.ops.ptmi.je_conv2d_pack(w[0], None, amax, geom, False))


def _wgrad_geom(cfg, C_in, C_out, KF, KT):
    """``ptmi_je_conv2d_wgrad``'s first 16 values with the roles exchanged: the written plane is the "input" under the taps, the block's
    input the pixel grid."""
    return [cfg.B, cfg.F_out, cfg.T_out, C_out, cfg.F_in, cfg.T_in, C_in, 1, KF, KT, *cfg.stride, *cfg.dilation, *cfg.front]


@lru_cache(maxsize=1024)
def _wgrad_width(cfg, C_in, C_out, KF, KT):
    """How many output channels one weight-gradient launch takes: the kernel stages the halo (here: of ``dz``) of every channel 64 of its
    columns touch, which at a large stride outgrows the LDS; then the columns are computed in halves (quarters, ...).  0: not even one."""
    lds = _lib.load().ptmi_je_conv2d_wgrad_lds
    width = C_out
    while lds(_lib.int64s(*_wgrad_geom(cfg, C_in, width, KF, KT), C_out)) < 1:
        if width == 1:
            return 0
        width = -(-width // 2)
    return width


def _wgrad(rows, dz, amax_rows, amax_d, cfg, C_in, C_out, KF, KT):
    """``dW [C_in, C_out, K_f, K_t]`` from ``rows`` (the block's input) and ``dz`` (on the written plane)."""
    width = _wgrad_width(cfg, C_in, C_out, KF, KT)
    slabs = wgrad_slabs(cfg.B, cfg.F_in, cfg.T_in, 1, C_in, width, KF * KT)
    parts = [torch.ops.ptmi.je_conv2d_wgrad(rows, None, dz[:, c:c + width], amax_rows, amax_d,
                                            _wgrad_geom(cfg, C_in, min(width, C_out - c), KF, KT), slabs)[0] for c in range(0, C_out, width)]
    return parts[0] if len(parts) == 1 else torch.cat(parts, 1)


class _BlockFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, residual, weight, bias, gate_weight, gate_bias, gamma, beta, slope, fixed, lengths, cfg):
        ops = torch.ops.ptmi
        B, per, act, p = cfg.B, cfg.norm == 'sequence', cfg.act, cfg.act_p
        C_in, C_out, KF, KT = weight.shape
        G = 1 if gate_weight is None else 2
        has_norm = cfg.norm is not None
        a, stats = x, None
        if cfg.pre:
            if has_norm:
                stats = fixed if fixed is not None else ops.je_conv_stats(x, lengths, B * cfg.F_in, cfg.T_in, per, cfg.eps)
            if has_norm or act:
                a = ops.je_conv_apply(x, None, None, stats, gamma, beta, lengths, slope, B * cfg.F_in, cfg.T_in, per, act, p)
        geom = plan(cfg, C_in, C_out, G)
        w_planes, amax_w = _planes_form(weight, gate_weight, geom)
        amax_a = _word(a)
        if cfg.pre or not has_norm:
            act_post = 0 if cfg.pre else act
            fused = bool(act_post) or G == 2 or residual is not None
            z, gz, out = ops.je_conv_transpose_forward(a, w_planes, amax_a, amax_w, bias, gate_bias, residual, slope, geom, act_post, p, fused)
            if not fused:
                out = z
        else:
            z, gz, _ = ops.je_conv_transpose_forward(a, w_planes, amax_a, amax_w, bias, gate_bias, None, None, geom, 0, 0., False)
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
        C_in, C_out, KF, KT = weight.shape
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
            # dW[ci, co, k] = sum over the input pixels i of a[i, ci] dz[i s + k d - front, co]: the weight gradient of a plain convolution
            # whose "output gradient" is a and whose "input" is dz - once per convolution, a is shared
            rows = a.contiguous()
            if need[2]:
                dw = _wgrad(rows, dz, amax_a, amax_d, cfg, C_in, C_out, KF, KT)
            if need[4]:
                dgw = _wgrad(rows, dgz, amax_a, amax_d, cfg, C_in, C_out, KF, KT)
        dx = None
        pre_stage = cfg.pre and (has_norm or bool(act))
        if need[0] or (pre_stage and want):
            # dx[i, ci] = sum over (k, co) of dz[i s + k d - front, co] W[ci, co, k]: je_conv2d_forward in mode 0 on the weights as they are
            geom = [B, cfg.F_out, cfg.T_out, C_out, 1, 1, 1, cfg.F_in, cfg.T_in, C_in, 1, KF, KT, *cfg.stride, *cfg.dilation, *cfg.front]
            planes, amax_w = _dx_planes_form(weight, geom)
            dx = ops.je_conv2d_forward(dz, None, planes, amax_d, amax_w, None, None, None, None, geom, 0, 0., False)[0]
            if G == 2:
                planes, amax_w = _dx_planes_form(gate_weight, geom)
                dx = ops.je_conv2d_forward(dgz, None, planes, amax_d, amax_w, None, None, dx, None, geom, 0, 0., True)[2]
            if pre_stage:
                dx, _, dparams = ops.je_conv_apply_backward(dx, x, None, stats, gamma, beta, lengths, slope, BI, cfg.T_in, per, ctx.fixed, act,
                                                            p, want)
        C = gamma.numel() if gamma is not None else (beta.numel() if beta is not None else 0)
        dgamma = dparams[:C].view(gamma.shape) if dparams is not None and gamma is not None and need[6] else None
        dbeta = dparams[dparams.numel() // 2:][:C].view(beta.shape) if dparams is not None and beta is not None and need[7] else None
        dslope = dparams[-1:].view(slope.shape) if dparams is not None and slope is not None and need[8] else None
        return (dx if need[0] else None, dout if need[1] else None, dw, db, dgw, dgb, dgamma, dbeta, dslope, None, None, None)


def conv_transpose_block(x, cfg, weight, bias=None, gate_weight=None, gate_bias=None, gamma=None, beta=None, slope=None, fixed=None,
                         lengths=None, residual=None):
    """One block on rows: ``x [B F_in T_in, C_in]`` -> ``(out [B F_out T_out, C_out], stats or None)``.  ``weight [C_in, C_out, K_f, K_t]``
    and ``gate_weight`` are the ``torch.nn.ConvTranspose2d`` parameters (a ``ConvTranspose1d``'s with ``K_f = 1``).  With a normalisation
    behind the convolution ``cfg`` describes the UNTRIMMED plane (``front = (0, 0)``) and ``lengths`` (``B F_out`` entries) are the
    trimmed ones, as the reference has it; the caller trims.  The rest as ``ops.je_conv2d.conv_block2d``."""
    _check('je_conv_transpose.conv_transpose_block', x, residual, weight, bias, gate_weight, gate_bias, gamma, beta, slope, fixed)
    if x.dim() != 2 or weight.dim() != 4 or x.shape != (cfg.B * cfg.F_in * cfg.T_in, weight.shape[0]):
        raise ValueError(f'je_conv_transpose.conv_transpose_block: x [{cfg.B * cfg.F_in * cfg.T_in}, {weight.shape[0]}], got {tuple(x.shape)}')
    if cfg.act == ACTIVATIONS['prelu'] and (slope is None or slope.numel() != 1):
        raise NotImplementedError('je_conv_transpose.conv_transpose_block: a PReLU with one parameter')
    C_in, C_out, KF, KT = weight.shape
    plan(cfg, C_in, C_out, 1)
    if torch.is_grad_enabled() and any(t is not None and t.requires_grad for t in (weight, gate_weight)):
        if _wgrad_width(cfg, C_in, C_out, KF, KT) < 1:
            raise NotImplementedError('je_conv_transpose.conv_transpose_block: the weight gradient of this geometry does not fit the LDS of '
                                      'a workgroup (the layer runs with weights that do not require a gradient): '
                                      f'{_wgrad_geom(cfg, C_in, C_out, KF, KT)}')
    cont = [None if t is None else t.contiguous() for t in (weight, bias, gate_weight, gate_bias)]
    flat = [None if t is None else t.reshape(-1) for t in (gamma, beta)]
    if cfg.norm is None:
        flat, fixed, lengths = [None, None], None, None
    return _BlockFn.apply(x, residual, *cont, *flat, slope, fixed, lengths, cfg)


class _UnpoolFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, index, geom):
        ctx.save_for_backward(index)
        ctx.geom = geom
        return torch.ops.ptmi.je_unpool_forward(x, index, geom)

    @staticmethod
    @once_differentiable
    def backward(ctx, dy):
        index, = ctx.saved_tensors
        return torch.ops.ptmi.je_unpool_backward(dy.contiguous(), index, ctx.geom), None, None


def unpool(x, index, geom):
    """``x [B F_in T_in, C]`` -> ``y [B F_out T_out, C]``; ``geom = (B, F_in, T_in, F_out, T_out, C, size f, t, stride f, t, front f, t)``.
    With ``index`` (int64 rows as ``pool2d`` returns them: positions on the padded and trimmed plane) output position ``p`` takes the
    value of the last window that names it, else zero; without, every value is repeated ``stride`` times."""
    _check('je_conv_transpose.unpool', x)
    if index is not None and not (index.is_cuda and index.dtype == torch.int64 and index.shape == x.shape):
        raise ValueError(f'je_conv_transpose.unpool: index int64 {tuple(x.shape)} on the GPU, got {index.dtype} {tuple(index.shape)}')
    return _UnpoolFn.apply(x, None if index is None else index.contiguous(), [int(v) for v in geom])
