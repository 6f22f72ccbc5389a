"""The WaveNet vocoder's operators on the HIP kernels of ``csrc/wavenet.hip`` and the planes GEMM (reference:
``padertorch/modules/wavenet/wavenet.py`` and nv-wavenet's sampling loop behind ``WaveNet.infer``).  Activations are ``[B, T, C]`` with
CHANNELS INNERMOST, as in ``ops/tcn.py``; fp32 on the GPU only.

    embed(audio, weight)                  mu-law codes and their embedding rows from one launch: (x0 [B, T, R], codes [B, T] int64)
    cond_upsample(features, weight, bias, stride, fading, out_len=None)
                                          the ConvTranspose1d of get_cond_input as GEMM + gather-form overlap-add (bias and crop fused)
    gate(P, bias, cond, dilation)         tanh(z[:R]) sigmoid(z[R:]) of one layer, z from P = x W^T, the bias and the conditioning slice
    tap_matrix(weight)                    the [2R, R, 2] dilated convolution as W [4R, R]: the tap on x[t - d] above the tap on x[t]
    residual_stack(x0, cond, dilations, dilate_w, dilate_b, res_w, res_b)
                                          all layers: per layer one GEMM, one gate launch, one residual GEMM -> acts_all [B, T, L, R]
    pack_inference(...), generate(...)    the weights in the sampling kernel's form and the sampling loop itself

All are differentiable where the reference is; every sum over rows is taken in one fixed order without atomics (``csrc/reduce.h``).
"""
import math

import torch
from torch.autograd.function import once_differentiable

from .. import _lib
from . import gemm as _gemm
from . import library  # noqa: F401  (registers torch.ops.ptmi.wavenet_*)

__all__ = ['embed', 'cond_upsample', 'crop_of', 'gate', 'tap_matrix', 'residual_stack', 'dilations_of', 'pack_inference', 'generate',
           'check_sizes', 'MAX_R', 'MAX_S', 'MAX_A', 'STEPS_PER_LAUNCH']

#: the sampling kernel's limits (``NotImplementedError`` beyond)
MAX_R, MAX_S, MAX_A = 256, 1024, 1024
#: time steps one launch of the sampling kernel covers by default: 176 - 189 us per step at R = 64, S = 256, A = 256, L = 16 on an MI355X
#: (``scripts/bench_wavenet.py``, ``profiles/wavenet.txt``: 527 - 566 steps in 100 ms)
STEPS_PER_LAUNCH = 512


def _check(name, *tensors):
    _lib.require_gpu(*tensors)
    for t in tensors:
        if t is not None and t.dtype != torch.float32:
            raise NotImplementedError(f'{name}: float32 only, got {t.dtype}')


def check_sizes(R, S, A):
    if not (1 <= R <= MAX_R and 1 <= S <= MAX_S and 2 <= A <= MAX_A):
        raise NotImplementedError(f'wavenet: the sampling kernel covers n_residual_channels <= {MAX_R}, n_skip_channels <= {MAX_S}, '
                                  f'n_out_channels <= {MAX_A}; got {R}, {S}, {A}')


def dilations_of(n_layers, max_dilation):
    """``2 ** (i % (floor(log2(max_dilation)) + 1))`` per layer (wavenet.py:115-117)."""
    loop = math.floor(math.log2(max_dilation)) + 1
    return [int(2 ** (i % loop)) for i in range(n_layers)]


# ------------------------------------------------------------------------------------------------ embedding
class _EmbedFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, audio, weight):
        codes, x0 = torch.ops.ptmi.wavenet_embed_forward(audio.contiguous(), weight.contiguous())
        ctx.save_for_backward(codes)
        ctx.A = weight.shape[0]
        ctx.mark_non_differentiable(codes)
        return x0, codes

    @staticmethod
    @once_differentiable
    def backward(ctx, g, _gcodes):
        codes, = ctx.saved_tensors
        return None, torch.ops.ptmi.wavenet_embed_backward(g.contiguous(), codes, ctx.A)


def embed(audio, weight):
    """``audio [B, T]`` in ``[-1, 1]``, ``weight [A, R]`` -> ``(x0 [B, T, R], codes [B, T] int64)``: ``codes = mu_law_encode(audio, A)``
    (clamped), ``x0 = weight[codes]``.  Differentiable in ``weight``."""
    _check('wavenet.embed', audio, weight)
    if audio.dim() != 2 or weight.dim() != 2 or audio.numel() == 0:
        raise ValueError(f'wavenet.embed: audio [B, T] and weight [A, R], got {tuple(audio.shape)}, {tuple(weight.shape)}')
    return _EmbedFn.apply(audio, weight)


# ------------------------------------------------------------------------------------------------ conditioning up-sampling
def crop_of(fading, window, stride):
    """``(front, back)`` columns the fading takes off the transposed convolution's output (wavenet.py:187-195)."""
    if fading not in ('full', 'half', None):
        raise ValueError(f"wavenet: fading 'full', 'half' or None, got {fading!r}")
    pad = window - stride
    if fading is None:
        return 0, 0
    if pad <= 0:
        raise ValueError(f'wavenet: fading {fading!r} needs upsamp_window > upsamp_stride (got {window}, {stride}): the crop [pad:-pad] is empty')
    return (pad, pad) if fading == 'full' else (pad // 2, math.ceil(pad / 2))


class _OlaFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, G, bias, B, Tf, window, stride, front, Tout):
        ctx.cfg = (Tf, window, stride, front)
        return torch.ops.ptmi.wavenet_ola_forward(G, bias.contiguous(), B, Tf, window, stride, front, Tout)

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        g = g.contiguous()
        need = ctx.needs_input_grad
        dG = torch.ops.ptmi.wavenet_ola_backward(g, *ctx.cfg) if need[0] else None
        db = torch.ops.ptmi.wavenet_colsum(g.view(-1, g.shape[2])) if need[1] else None
        return dG, db, None, None, None, None, None, None


class _MmFn(torch.autograd.Function):
    """``x [M, K] @ w [K, N]`` with both gradients: three calls of ``ops.gemm.mm``."""

    @staticmethod
    def forward(ctx, x, w):
        ctx.save_for_backward(x, w)
        return _gemm.mm(x, w)

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        x, w = ctx.saved_tensors
        g = g.contiguous()
        need = ctx.needs_input_grad
        return (_gemm.mm(g, w.t()) if need[0] else None), (_gemm.mm(x.t(), g) if need[1] else None)


def cond_upsample(features, weight, bias, stride, fading='full', out_len=None):
    """``ConvTranspose1d(C, C, window, stride)`` and the fading crop: ``features [B, C, Tf]``, ``weight [C, C, window]``, ``bias [C]`` ->
    ``[B, Tout, C]`` (channels innermost).  ``out_len``: only the first ``out_len`` columns are computed."""
    _check('wavenet.cond_upsample', features, weight, bias)
    if features.dim() != 3 or weight.dim() != 3 or weight.shape[0] != features.shape[1] or tuple(bias.shape) != (weight.shape[1],):
        raise ValueError(f'wavenet.cond_upsample: features [B, C, Tf], weight [C, C2, window], bias [C2], got {tuple(features.shape)}, '
                         f'{tuple(weight.shape)}, {tuple(bias.shape)}')
    B, C, Tf = features.shape
    C2, window = weight.shape[1], weight.shape[2]
    front, back = crop_of(fading, window, stride)
    full = (Tf - 1) * stride + window
    Tout = full - front - back
    if out_len is not None:
        if out_len > Tout:
            raise ValueError(f'wavenet.cond_upsample: {out_len} columns asked for, {Tout} exist')
        Tout = int(out_len)
    if Tf < 1 or Tout < 1:
        raise ValueError(f'wavenet.cond_upsample: no output columns for {Tf} frames, window {window}, stride {stride}, fading {fading!r}')
    rows = features.transpose(1, 2).reshape(B * Tf, C)
    G = _MmFn.apply(rows, weight.reshape(C, C2 * window))
    return _OlaFn.apply(G, bias, B, Tf, window, int(stride), front, Tout)


# ------------------------------------------------------------------------------------------------ gate
class _GateFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, P, bias, cond, dilation):
        P, bias = P.contiguous(), bias.contiguous()
        B, T, R4 = P.shape
        acts = torch.empty((B, T, R4 // 4), dtype=torch.float32, device=P.device)
        torch.ops.ptmi.wavenet_gate_forward_(acts, P, bias, cond, dilation)
        ctx.save_for_backward(P, bias, cond)
        ctx.dilation = dilation
        return acts

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        P, bias, cond = ctx.saved_tensors
        need = ctx.needs_input_grad
        B, T, R4 = P.shape
        dz = torch.empty((B, T, R4 // 2), dtype=torch.float32, device=P.device)
        dP, db = torch.ops.ptmi.wavenet_gate_backward_(dz, g.contiguous(), P, bias, cond, ctx.dilation, need[0], need[1])
        return (dP if need[0] else None), (db if need[1] else None), (dz if need[2] else None), None


def _even_rows(t):
    return t.stride(2) == 1 and (t.shape[0] == 1 or t.stride(0) == t.shape[1] * t.stride(1))


def gate(P, bias, cond, dilation):
    """One layer's gated activation: ``P [B, T, 4R]`` (``x W^T`` with :func:`tap_matrix`), ``bias [2R]``, ``cond [B, T, 2R]`` (may be a
    channel slice of a wider ``[B, T, L 2R]`` tensor, read in place) -> ``acts [B, T, R]``."""
    _check('wavenet.gate', P, bias, cond)
    if P.dim() != 3 or P.shape[2] % 4 or cond.dim() != 3 or tuple(cond.shape) != (P.shape[0], P.shape[1], P.shape[2] // 2) \
            or bias.numel() != P.shape[2] // 2 or dilation < 1 or P.numel() == 0:
        raise ValueError(f'wavenet.gate: P [B, T, 4R], bias [2R], cond [B, T, 2R], got {tuple(P.shape)}, {tuple(bias.shape)}, {tuple(cond.shape)}')
    if not _even_rows(cond):
        cond = cond.contiguous()
    return _GateFn.apply(P, bias, cond, int(dilation))


def tap_matrix(weight):
    """``Conv1d(R, 2R, kernel_size=2).weight [2R, R, 2]`` -> ``W [4R, R]``: ``weight[:, :, 0]`` (the tap on ``x[t - d]``) above
    ``weight[:, :, 1]`` (the tap on ``x[t]``)."""
    return torch.cat((weight[:, :, 0], weight[:, :, 1]), 0)


# ------------------------------------------------------------------------------------------------ the residual stack
class _StackFn(torch.autograd.Function):
    """Inputs: ``x0 [B, T, R]``, ``cond [B, T, L 2R]``, ``dilations``, then ``L`` dilated weights ``[2R, R, 2]``, ``L`` biases ``[2R]``,
    ``L - 1`` residual weights ``[R, R, 1]`` and ``L - 1`` biases ``[R]``.  Saves per layer the input ``x_l`` and ``P_l``; the backward
    recomputes ``z``, writes ``dz`` into slice ``l`` of ONE ``dcond`` buffer and adds the residual path's gradient into slice ``l`` of its
    copy of ``dacts_all``."""

    @staticmethod
    def forward(ctx, x0, cond, dilations, *params):
        L = len(dilations)
        dw, db, rw, rb = params[:L], params[L:2 * L], params[2 * L:3 * L - 1], params[3 * L - 1:]
        B, T, R = x0.shape
        x = x0.contiguous().view(B * T, R)
        cond = cond.contiguous()
        acts_all = torch.empty((B, T, L, R), dtype=torch.float32, device=x0.device)
        flat = acts_all.view(B * T, L * R)
        xs, Ps, Ws = [], [], []
        for l in range(L):
            W = tap_matrix(dw[l])
            P = _gemm.mm(x, W.t()).view(B, T, 4 * R)
            torch.ops.ptmi.wavenet_gate_forward_(acts_all[:, :, l], P, db[l].contiguous(), cond[:, :, l * 2 * R:(l + 1) * 2 * R], dilations[l])
            xs.append(x), Ps.append(P), Ws.append(W)
            if l < L - 1:
                x = _gemm.mm(flat[:, l * R:(l + 1) * R], rw[l].view(R, R).t(), bias=rb[l], out=x.clone(), accumulate=True,
                             amax_x=_gemm.UNIT_RANGE)
        ctx.save_for_backward(cond, acts_all, *xs, *Ps, *Ws, *db, *rw)
        ctx.dilations, ctx.shape = tuple(dilations), (B, T, R, L)
        return acts_all

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        B, T, R, L = ctx.shape
        saved = ctx.saved_tensors
        cond, acts_all = saved[:2]
        xs, Ps, Ws = saved[2:2 + L], saved[2 + L:2 + 2 * L], saved[2 + 2 * L:2 + 3 * L]
        db, rw = saved[2 + 3 * L:2 + 4 * L], saved[2 + 4 * L:]
        need = ctx.needs_input_grad
        n_dw, n_db, n_rw, n_rb = (need[3:3 + L], need[3 + L:3 + 2 * L], need[3 + 2 * L:3 + 3 * L - 1], need[3 + 3 * L - 1:])
        dacts = g.clone(memory_format=torch.contiguous_format)
        dflat = dacts.view(B * T, L * R)
        aflat = acts_all.view(B * T, L * R)
        dcond = torch.empty_like(cond)
        g_dw, g_db, g_rw, g_rb = [None] * L, [None] * L, [None] * (L - 1), [None] * (L - 1)
        dx = None
        for l in reversed(range(L)):
            sl = slice(l * R, (l + 1) * R)
            if l < L - 1 and dx is not None:
                if n_rw[l]:
                    g_rw[l] = _gemm.mm(dx.t(), aflat[:, sl], amax_y=_gemm.UNIT_RANGE).view(R, R, 1)
                if n_rb[l]:
                    g_rb[l] = torch.ops.ptmi.wavenet_colsum(dx)
                _gemm.mm(dx, rw[l].view(R, R), out=dflat[:, sl], accumulate=True)
            dP, dbias = torch.ops.ptmi.wavenet_gate_backward_(dcond[:, :, l * 2 * R:(l + 1) * 2 * R], dacts[:, :, l], Ps[l], db[l].contiguous(),
                                                              cond[:, :, l * 2 * R:(l + 1) * 2 * R], ctx.dilations[l], True, bool(n_db[l]))
            dP = dP.view(B * T, 4 * R)
            if n_db[l]:
                g_db[l] = dbias
            if n_dw[l]:
                dW = _gemm.mm(dP.t(), xs[l])
                g_dw[l] = torch.stack((dW[:2 * R], dW[2 * R:]), 2)
            if l > 0 or need[0]:
                # x_{l+1} = x_l + residual: the gradient buffer is carried down the stack and every layer adds its dP W
                dx = _gemm.mm(dP, Ws[l]) if dx is None else _gemm.mm(dP, Ws[l], out=dx, accumulate=True)
        return ((dx.view(B, T, R) if need[0] else None), (dcond if need[1] else None), None, *g_dw, *g_db, *g_rw, *g_rb)


def residual_stack(x0, cond, dilations, dilate_w, dilate_b, res_w, res_b):
    """The ``L`` gated layers (wavenet.py:151-159): ``x0 [B, T, R]``, ``cond [B, T, L 2R]`` (the output of ``cond_layers``, layer-major
    channels), per layer ``dilate_w [2R, R, 2]``, ``dilate_b [2R]`` and, for all but the last, ``res_w [R, R, 1]``, ``res_b [R]`` ->
    ``acts_all [B, T, L, R]``.  The skip sum is one GEMM on ``acts_all.view(B, T, L R)``."""
    L = len(dilations)
    _check('wavenet.residual_stack', x0, cond, *dilate_w, *dilate_b, *res_w, *res_b)
    if not (len(dilate_w) == len(dilate_b) == L and len(res_w) == len(res_b) == L - 1 and L >= 1):
        raise ValueError(f'wavenet.residual_stack: {L} layers need {L} dilated and {L - 1} residual convolutions')
    if x0.dim() != 3 or x0.numel() == 0 or tuple(cond.shape) != (x0.shape[0], x0.shape[1], 2 * L * x0.shape[2]):
        raise ValueError(f'wavenet.residual_stack: x0 [B, T, R] and cond [B, T, L 2R], got {tuple(x0.shape)}, {tuple(cond.shape)}')
    R = x0.shape[2]
    for w, b in zip(dilate_w, dilate_b):
        if tuple(w.shape) != (2 * R, R, 2) or tuple(b.shape) != (2 * R,):
            raise ValueError(f'wavenet.residual_stack: dilated convolution [2R, R, 2] / [2R], got {tuple(w.shape)}, {tuple(b.shape)}')
    for w, b in zip(res_w, res_b):
        if tuple(w.shape) != (R, R, 1) or tuple(b.shape) != (R,):
            raise ValueError(f'wavenet.residual_stack: residual convolution [R, R, 1] / [R], got {tuple(w.shape)}, {tuple(b.shape)}')
    return _StackFn.apply(x0, cond, [int(d) for d in dilations], *dilate_w, *dilate_b, *res_w, *res_b)


# ------------------------------------------------------------------------------------------------ sampling
def pack_inference(dilate_w, dilate_b, res_w, res_b, skip_w, skip_b, conv_out_w, conv_end_w):
    """The weights in the sampling kernel's form (one flat fp32 tensor; include/ptmi.h ``ptmi_wavenet_generate``): every matrix transposed
    so that a thread's output column is contiguous across the lanes, the dilated taps stacked along k, skip and residual side by side (the
    last layer's residual columns zero)."""
    L = len(dilate_w)
    R = dilate_w[0].shape[1]
    S = skip_w[0].shape[0]
    parts = []
    with torch.no_grad():
        for l in range(L):
            parts += [tap_matrix(dilate_w[l]).view(2, 2 * R, R).permute(0, 2, 1).reshape(-1), dilate_b[l].reshape(-1)]
            rs_w = torch.zeros((R, S + R), dtype=torch.float32, device=dilate_w[0].device)
            rs_b = torch.zeros(S + R, dtype=torch.float32, device=dilate_w[0].device)
            rs_w[:, :S], rs_b[:S] = skip_w[l].view(S, R).t(), skip_b[l]
            if l < L - 1:
                rs_w[:, S:], rs_b[S:] = res_w[l].view(R, R).t(), res_b[l]
            parts += [rs_w.reshape(-1), rs_b]
        parts += [conv_out_w.view(conv_out_w.shape[0], S).t().reshape(-1), conv_end_w.view(conv_end_w.shape[0], -1).t().reshape(-1)]
        return torch.cat(parts).contiguous()


def chunks_of(length, chunk_length, chunk_overlap):
    """``[(onset, length)]`` of the independent restarts of ``WaveNet.infer`` (wavenet.py:256-269)."""
    if chunk_length is None or length <= chunk_length:
        return [(0, length)]
    n = math.ceil((length - chunk_overlap) / (chunk_length - chunk_overlap))
    chunk_length = math.ceil(length / n) + chunk_overlap
    return [(on, min(chunk_length, length - on)) for on in range(0, length - chunk_overlap, chunk_length - chunk_overlap)]


def generate(packed, embed_w, cond, selectors, dilations, S, A, chunks=None, steps_per_launch=None, return_logits=False):
    """The sampling loop: ``cond [B, T, L 2R]`` (``cond_layers`` of the up-sampled features), ``selectors [B, T]`` uniforms in ``[0, 1)``,
    ``chunks [(onset, length)]`` (default: the whole length) -> per chunk a ``codes [B, length] int64`` (and ``logits [B, length, A]``).
    Every (example, chunk) pair is a sequence of its own in the SAME launches; at step ``t`` a sequence embeds its previous code
    (``A // 2`` at ``t = 0``), reads conditioning column ``onset + t`` and draws with ``selectors[b, onset + t]``."""
    _check('wavenet.generate', packed, embed_w, cond, selectors)
    L = len(dilations)
    R = embed_w.shape[1]
    check_sizes(R, S, A)
    if cond.dim() != 3 or cond.shape[2] != 2 * R * L or cond.numel() == 0:
        raise ValueError(f'wavenet.generate: cond [B, T, L 2R = {2 * R * L}], got {tuple(cond.shape)}')
    if tuple(selectors.shape) != tuple(cond.shape[:2]):
        raise ValueError(f'wavenet.generate: selectors {tuple(cond.shape[:2])}, got {tuple(selectors.shape)}')
    if embed_w.shape[0] < A:
        raise NotImplementedError(f'wavenet.generate: {A} output classes are fed back into an embedding of {embed_w.shape[0]} rows')
    B, T = selectors.shape
    chunks = [(0, T)] if chunks is None else [(int(o), int(n)) for o, n in chunks]
    if any(o < 0 or n < 1 or o + n > T for o, n in chunks):
        raise ValueError(f'wavenet.generate: chunks {chunks} outside [0, {T})')
    steps = int(steps_per_launch or STEPS_PER_LAUNCH)
    if steps < 1:
        raise ValueError(f'wavenet.generate: steps_per_launch {steps_per_launch!r}')
    dev = cond.device
    lib = _lib.load()
    ex = lib.ptmi_wavenet_generate_ex()
    seqs = [(b, o, n) for o, n in chunks for b in range(B)]
    nseq, Tmax = len(seqs), max(n for _, n in chunks)
    groups = -(-nseq // ex)
    firsts, rows = [], 0
    for d in dilations:
        firsts.append(rows)
        rows += int(d)
    layer_meta = _lib.host_to_device([v for d, f in zip(dilations, firsts) for v in (int(d), f)], torch.int32, dev).view(L, 2)
    seq_meta = _lib.host_to_device([v for s in seqs for v in s], torch.int32, dev).view(nseq, 3)
    ring = torch.zeros(groups * rows * ex * R, dtype=torch.float32, device=dev)
    last = torch.full((groups * ex,), A // 2, dtype=torch.int32, device=dev)
    y = torch.zeros((nseq, Tmax), dtype=torch.int64, device=dev)
    logits = torch.zeros((nseq, Tmax, A), dtype=torch.float32, device=dev) if return_logits else None
    cond, selectors = cond.contiguous(), selectors.contiguous()
    for t0 in range(0, Tmax, steps):
        torch.ops.ptmi.wavenet_generate_(y, logits, ring, last, packed, embed_w.contiguous(), cond, selectors, layer_meta, seq_meta, S, A, rows,
                                         t0, min(steps, Tmax - t0))
    out = []
    for c, (_, n) in enumerate(chunks):
        codes = y[c * B:(c + 1) * B, :n]
        out.append((codes, logits[c * B:(c + 1) * B, :n]) if return_logits else codes)
    return out
