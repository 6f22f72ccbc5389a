"""The HIP kernels of the hot path as registered torch custom ops (``torch.ops.ptmi.*``).

Every op is a thin CUDA-dispatch-key implementation over one entry point (or a fixed pair) of the C ABI in
``include/ptmi.h`` / ``libptmi.so``: tensors in, tensors out, launch on torch's current stream.  They carry no
autograd formula of their own: the differentiable operators (``ops.STFT``, ``ops.pit_features``, ``ops.gemm.mm``,
``ops.packed_lstm``, the loss functions) are ``torch.autograd.Function`` s whose forward and backward call these ops, so
a forward kernel and its hand-written adjoint kernel stay paired.  There is no CPU implementation: calling an op
with CPU tensors fails in the dispatcher (``NotImplementedError: ... 'CPU' backend``).

    torch.ops.ptmi.stft_forward            ptmi_stft_forward                  (padertorch/ops/_stft.py:103-174)
    torch.ops.ptmi.istft_forward           ptmi_istft_forward                 (_stft.py:176-263)
    torch.ops.ptmi.pit_features            ptmi_pit_features                  (pit/data.py:49-77)
    torch.ops.ptmi.pit_loss_forward        ptmi_pit_pairwise_sse + _assign    (ops/losses/source_separation.py:34-312)
    torch.ops.ptmi.pit_loss_backward       ptmi_pit_backward
    torch.ops.ptmi.dc_loss_forward / _backward     ptmi_dc_loss_*             (source_separation.py:13-31)
    torch.ops.ptmi.unit_norm_forward / _backward   ptmi_unit_norm_*           (contrib/tcl/dc.py:70)
    torch.ops.ptmi.lstm_recurrence_forward / _backward   ptmi_lstm_*_persistent, falling back to ptmi_lstm_forward / _backward
                                                                              (torch.nn.LSTM in pit/model.py:60-66,97)
    torch.ops.ptmi.absmax                          ptmi_absmax                (operand scale of the dense layers' fp32 operands)
    torch.ops.ptmi.pack_planes_t / _n, torch.ops.ptmi.gemm_planes_   ptmi_pack_planes_t / _n, ptmi_gemm_planes   (nn.LSTM input projections, nn.Linear, all their gradients)
    torch.ops.ptmi.pack_planes_bf16_list, torch.ops.ptmi.gemm_planes_bf16_group_   ptmi_pack_planes_t_bf16_list, ptmi_gemm_planes_bf16_group
                                                                              (one BLSTM layer's four weight gradients, one launch)
    torch.ops.ptmi.lstm_weight_prep                ptmi_lstm_weight_prep      (the nn.LSTM parameters' operand forms, once per optimizer step)
    torch.ops.ptmi.grad_norm, torch.ops.ptmi.adam_flat_  ptmi_grad_norm, ptmi_adam_flat (train/optimizer.py:27-42, trainer.py:512-532)
    torch.ops.ptmi.tas_analysis / tas_synthesis / tas_masked_decode_backward / tas_wgrad   ptmi_tas_*
                                                                              (tasnet/tas_coders.py:9-135, tasnet/model.py:119-129)
    torch.ops.ptmi.tcn_depthwise_forward / _backward, tcn_norm_stats / _apply / _backward   ptmi_tcn_*   (modules/convnet.py:114-161)
    torch.ops.ptmi.tasnet_entry_norm_forward / _backward, tasnet_prelu_forward / _backward, tasnet_mask_head_forward / _backward,
    torch.ops.ptmi.tasnet_center           ptmi_tasnet_*                      (tasnet/model.py:86-142)
    torch.ops.ptmi.td_rect_stats / td_rect_lincomb / orpit_select   ptmi_td_rect_*, ptmi_orpit_select   (or_pit/model.py:58-98,319-350)
    torch.ops.ptmi.orpit_flag_forward / _backward  ptmi_orpit_flag_*          (or_pit/model.py:187-218)
    torch.ops.ptmi.dprnn_tables / chunk_lstm_forward / chunk_lstm_backward / dprnn_colsum / dprnn_colsum_pair / dprnn_norm_residual_forward / _backward /
    torch.ops.ptmi.dprnn_segment / dprnn_overlap_add   ptmi_dprnn_*, ptmi_chunk_lstm_*   (modules/dual_path_rnn.py)
    torch.ops.ptmi.bf_psd / bf_souden / bf_apply / bf_eig / bf_ban / bf_phase   ptmi_bf_*   (mask_estimator/evaluate.py:110-137,
                                                                              jensheit/evaluation.py:14-45)
    torch.ops.ptmi.mask_loss_forward / _backward   ptmi_mask_loss_*          (jensheit/mask_estimator_example/model.py:128-237)
    torch.ops.ptmi.gl_project / gl_project_backward / gl_update / gl_iterations   ptmi_gl_*   (contrib/mk/synthesis/parametric/griffin_lim.py:32-156)
    torch.ops.ptmi.anti_alias_forward / _backward  ptmi_anti_alias_*         (contrib/mk/synthesis/vocoder/nvidia_bigvgan/alias_free_activation/torch,
                                                                              nvidia_bigvgan/activations.py)
    torch.ops.ptmi.mu_law_encode / _decode, wavenet_embed_forward / _backward, wavenet_ola_forward / _backward, wavenet_gate_forward_ /
    _backward_, wavenet_colsum, wavenet_generate_   ptmi_mu_law_*, ptmi_wavenet_*   (ops/mu_law.py, modules/wavenet/wavenet.py, nv_wavenet)
    torch.ops.ptmi.bigvgan_taps_ / bigvgan_conv_direct_ / bigvgan_ola / bigvgan_post   ptmi_bigvgan_*   (contrib/mk/synthesis/vocoder/
                                                                              nvidia_bigvgan/bigvgan.py: the generator's convolutions)
    torch.ops.ptmi.attn_forward / attn_weights / attn_backward, transformer_posenc_, transformer_norm_residual_forward / _backward
                                                   ptmi_attn_*, ptmi_transformer_*   (contrib/je/modules/transformer.py:12-38,151-174,234-243)
    torch.ops.ptmi.chunk_gru_forward / chunk_gru_backward, seq_table, seq_gather, seq_pool_forward / _backward
                                                   ptmi_chunk_gru_*, ptmi_seq_*   (contrib/je/modules/rnn.py, reduce.py)
    torch.ops.ptmi.je_conv_taps / je_conv_dtaps / je_conv_stats / je_conv_apply / je_conv_apply_backward, je_pool_forward / _backward
                                                   ptmi_je_conv_*, ptmi_je_pool_*   (contrib/je/modules/conv.py, conv_utils.py)
"""
import ctypes
from typing import List, Optional, Tuple

import torch
from torch import Tensor

from .. import _lib

_LIBRARY = torch.library.Library('ptmi', 'DEF')


def _register(schema):
    """``schema``: 'name(args) -> ret' in the dispatcher's schema language; the decorated function becomes the CUDA kernel."""
    name = schema.split('(', 1)[0].strip()

    def deco(fn):
        _LIBRARY.define(schema)
        _LIBRARY.impl(name, fn, 'CUDA')
        return getattr(torch.ops.ptmi, name)
    return deco


def _geom(g: List[int]):
    return _lib.StftGeom(*[int(v) for v in g])


# ------------------------------------------------------------------------------------------------ STFT front-end
@_register('stft_forward(Tensor x, Tensor? row_samples, Tensor window, Tensor twiddle, int[] geom, int frames, int layout, '
           'float edge_scale, str timer) -> Tensor')
def stft_forward(x, row_samples, window, twiddle, geom, frames, layout, edge_scale, timer):
    rows, T = x.shape
    F = geom[0] // 2 + 1
    shape = (rows, frames, F, 2) if layout == 0 else (rows, frames, 2 * F)
    out = torch.empty(shape, dtype=torch.float32, device=x.device)
    _lib.call('ptmi_stft_forward', x.data_ptr(), rows, x.stride(0), T, _lib.ptr(row_samples), window.data_ptr(), twiddle.data_ptr(),
              _geom(geom), frames, layout, edge_scale, out.data_ptr(), _lib.stream(x.device), timer=timer)      # '': not timed
    return out


@_register('istft_forward(Tensor spec, Tensor window, Tensor twiddle, int[] geom, int layout, float edge_scale, int cut_left, '
           'int out_samples, str timer) -> Tensor')
def istft_forward(spec, window, twiddle, geom, layout, edge_scale, cut_left, out_samples, timer):
    rows, frames = spec.shape[0], spec.shape[1]
    out = torch.empty((rows, max(out_samples, 0)), dtype=torch.float32, device=spec.device)
    if out_samples > 0:
        _lib.call('ptmi_istft_forward', spec.data_ptr(), rows, frames, None, window.data_ptr(), twiddle.data_ptr(), _geom(geom), layout,
                  edge_scale, cut_left, out_samples, out_samples, out.data_ptr(), _lib.stream(spec.device), timer=timer)
    return out


@_register('pit_features(Tensor y, Tensor? s, Tensor? num_samples, Tensor window, Tensor twiddle, int[] geom, int frames) '
           '-> (Tensor, Tensor?, Tensor?)')
def pit_features(y, s, num_samples, window, twiddle, geom, frames):
    return _pit_features(y, s, num_samples, window, twiddle, geom, frames, None, None, None)


@_register('pit_features_packed(Tensor y, Tensor? s, Tensor? num_samples, Tensor window, Tensor twiddle, int[] geom, int frames, '
           'Tensor(a!) log1p_packed, Tensor(b!)? log1p_planes, Tensor? packed_offsets) -> (Tensor, Tensor?, Tensor?)')
def pit_features_packed(y, s, num_samples, window, twiddle, geom, frames, log1p_packed, log1p_planes, packed_offsets):
    """``pit_features`` that also writes the first BLSTM layer's input: ``log1p(Y_abs)`` as PackedSequence rows (fp32, and as fp16
    planes in ``log1p_planes`` - zeroed once by the caller, the kernel never writes the padding)."""
    return _pit_features(y, s, num_samples, window, twiddle, geom, frames, log1p_packed, log1p_planes, packed_offsets)


def _pit_features(y, s, num_samples, window, twiddle, geom, frames, log1p_packed, log1p_planes, packed_offsets):
    B, N = y.shape
    K = s.shape[1] if s is not None else 0
    F = geom[0] // 2 + 1
    dev = y.device
    Y_abs = torch.empty((B, frames, F), dtype=torch.float32, device=dev)
    X_abs = cos_pd = None
    if K:
        X_abs = torch.empty((B, frames, K, F), dtype=torch.float32, device=dev)
        cos_pd = torch.empty((B, frames, K, F), dtype=torch.float32, device=dev)
    rc = _lib.call('ptmi_pit_features_packed', y.data_ptr(), _lib.ptr(s), B, K, N, N, _lib.ptr(num_samples), window.data_ptr(),
                   twiddle.data_ptr(), _geom(geom), frames, Y_abs.data_ptr(), _lib.ptr(X_abs), _lib.ptr(cos_pd), _lib.ptr(log1p_packed),
                   _lib.ptr(log1p_planes), _lib.ptr(packed_offsets), _lib.stream(dev), timer='pit_features', accept=(-2,))
    if rc == -2:
        raise NotImplementedError(f'pit_features: STFT size {geom[0]} / window {geom[2]} beyond what the direct-DFT kernel stages in LDS')
    return Y_abs, X_abs, cos_pd


# ------------------------------------------------------------------------------------------------ losses
@_register('pit_loss_forward(Tensor est, Tensor? obs, Tensor tgt, Tensor? scale, Tensor? row_frames, int B, int T, int K, int F, '
           'int[] strides) -> (Tensor, Tensor, Tensor, Tensor)')
def pit_loss_forward(est, obs, tgt, scale, row_frames, B, T, K, F, strides):
    lib = _lib.load()
    dev = est.device
    nvar = 2 if scale is not None else 1
    ws = torch.empty(int(lib.ptmi_pit_workspace_elems(B, T, K, F)), dtype=torch.float64, device=dev)
    sse = torch.empty((B, nvar, K, K), dtype=torch.float64, device=dev)
    st = _lib.stream(dev)
    _lib.call('ptmi_pit_pairwise_sse', est.data_ptr(), _lib.ptr(obs), tgt.data_ptr(), _lib.ptr(scale), B, T, _lib.int64s(*strides), K, F,
              _lib.ptr(row_frames), ws.data_ptr(), sse.data_ptr(), st, timer='pit_pairwise_sse')
    loss = torch.empty(nvar, dtype=torch.float32, device=dev)
    perm = torch.empty((B, nvar, K), dtype=torch.int32, device=dev)
    ex_loss = torch.empty((B, nvar), dtype=torch.float32, device=dev)
    _lib.call('ptmi_pit_assign', sse.data_ptr(), B, nvar, K, F, T, _lib.ptr(row_frames), loss.data_ptr(), perm.data_ptr(),
              ex_loss.data_ptr(), st)
    return loss, perm, ex_loss, sse


@_register('pit_loss_backward(Tensor est, Tensor? obs, Tensor tgt, Tensor? scale, Tensor perm, Tensor g_loss, Tensor? row_frames, '
           'int B, int T, int K, int F, int[] strides) -> Tensor')
def pit_loss_backward(est, obs, tgt, scale, perm, g_loss, row_frames, B, T, K, F, strides):
    nvar = 2 if scale is not None else 1
    # the kernel writes every (b, t < T) row, zero for the padded frames t >= T_b
    grad = torch.empty_strided(est.shape, est.stride(), dtype=est.dtype, device=est.device)
    _lib.call('ptmi_pit_backward', est.data_ptr(), _lib.ptr(obs), tgt.data_ptr(), _lib.ptr(scale), perm.data_ptr(), g_loss.data_ptr(), B, T,
              _lib.int64s(*strides), K, F, nvar, _lib.ptr(row_frames), grad.data_ptr(), _lib.stream(est.device), timer='pit_backward')
    return grad


@_register('dc_loss_forward(Tensor x, Tensor t, Tensor? row_frames, int B, int T, int E, int K, int F, int[] strides) '
           '-> (Tensor, Tensor, Tensor)')
def dc_loss_forward(x, t, row_frames, B, T, E, K, F, strides):
    lib = _lib.load()
    dev = x.device
    ws = torch.empty(int(lib.ptmi_dc_workspace_elems(B, T, F)), dtype=torch.float32, device=dev)
    gram = torch.empty((B, 32, 32), dtype=torch.float64, device=dev)
    ex_loss = torch.empty(B, dtype=torch.float32, device=dev)
    loss = torch.empty(1, dtype=torch.float32, device=dev)
    _lib.call('ptmi_dc_loss_forward', x.data_ptr(), t.data_ptr(), B, T, _lib.int64s(*strides), E, K, F, _lib.ptr(row_frames),
              ws.data_ptr(), gram.data_ptr(), ex_loss.data_ptr(), loss.data_ptr(), _lib.stream(dev), timer='dc_loss_forward')
    return loss, ex_loss, gram


@_register('dc_loss_backward(Tensor x, Tensor t, Tensor gram, Tensor g_loss, Tensor? row_frames, int B, int T, int E, int K, int F, '
           'int[] strides, bool zero_fill) -> Tensor')
def dc_loss_backward(x, t, gram, g_loss, row_frames, B, T, E, K, F, strides, zero_fill):
    dx = torch.zeros_like(x, memory_format=torch.preserve_format) if zero_fill \
        else torch.empty_strided(x.shape, x.stride(), dtype=x.dtype, device=x.device)
    _lib.call('ptmi_dc_loss_backward', x.data_ptr(), t.data_ptr(), gram.data_ptr(), g_loss.data_ptr(), B, T, _lib.int64s(*strides), E, K,
              F, _lib.ptr(row_frames), dx.data_ptr(), _lib.stream(x.device), timer='dc_loss_backward')
    return dx


# ------------------------------------------------------------------------------------------------ TasNet learned-basis coders
def _tas_dims(feat, weight):
    B, N, E = feat.shape
    assert weight.shape[0] == N and weight.is_contiguous() and feat.is_contiguous(), (feat.shape, weight.shape)
    return B, N, E, weight.numel() // N


@_register('tas_analysis(Tensor x, Tensor weight, Tensor? bias, int stride, int frames, bool relu) -> Tensor')
def tas_analysis(x, weight, bias, stride, frames, relu):
    """``x [B, T]``, ``weight [N, (1,) L]`` -> ``act(conv1d(x, weight, stride) + bias) [B, N, frames]``; ``x`` reads as zero from ``T`` on
    (``ptmi_tas_analysis``)."""
    B, T = x.shape
    N = weight.shape[0]
    L = weight.numel() // N
    assert x.is_contiguous() and weight.is_contiguous()
    out = torch.empty((B, N, frames), dtype=torch.float32, device=x.device)
    _lib.call('ptmi_tas_analysis', x.data_ptr(), weight.data_ptr(), _lib.ptr(bias), out.data_ptr(), B, T, N, L, stride, frames, int(relu),
              _lib.stream(x.device), timer='tas_analysis')
    return out


@_register('tas_synthesis(Tensor p, Tensor? mask, Tensor? gate, Tensor weight, Tensor? bias, int stride, int samples) -> Tensor')
def tas_synthesis(p, mask, gate, weight, bias, stride, samples):
    """``conv_transpose1d`` of ``p [B, N, E]`` (of ``mask[k] * p`` for every ``k`` with ``mask [K, B, N, E]``; of ``p * (gate > 0)`` with
    ``gate``), cut to ``samples``: ``[B, samples]``, with ``mask`` ``[K, B, samples]`` (``ptmi_tas_synthesis``)."""
    B, N, E, L = _tas_dims(p, weight)
    K = 1
    if mask is not None:
        K = mask.shape[0]
        assert mask.shape == (K, B, N, E) and mask.is_contiguous(), mask.shape
    assert gate is None or (gate.shape == p.shape and gate.is_contiguous())
    y = torch.empty((B, samples) if mask is None else (K, B, samples), dtype=torch.float32, device=p.device)
    _lib.call('ptmi_tas_synthesis', p.data_ptr(), _lib.ptr(mask), _lib.ptr(gate), weight.data_ptr(), _lib.ptr(bias), y.data_ptr(), K, B, N,
              L, stride, E, samples, _lib.stream(p.device), timer='tas_synthesis')
    return y


@_register('tas_masked_decode_backward(Tensor gy, Tensor mask, Tensor encoded, Tensor weight, int stride) -> (Tensor, Tensor)')
def tas_masked_decode_backward(gy, mask, encoded, weight, stride):
    """``(dmask, dencoded)`` of ``y[k] = conv_transpose1d(mask[k] * encoded)`` for ``gy [K, B, T]`` (``ptmi_tas_masked_decode_backward``)."""
    B, N, E, L = _tas_dims(encoded, weight)
    K, _, T = gy.shape
    assert mask.shape == (K, B, N, E) and gy.shape[1] == B and mask.is_contiguous() and gy.is_contiguous(), (mask.shape, gy.shape)
    dmask, denc = torch.empty_like(mask), torch.empty_like(encoded)
    _lib.call('ptmi_tas_masked_decode_backward', gy.data_ptr(), mask.data_ptr(), encoded.data_ptr(), weight.data_ptr(), dmask.data_ptr(),
              denc.data_ptr(), K, B, T, N, L, stride, E, _lib.stream(gy.device), timer='tas_masked_decode_backward')
    return dmask, denc


@_register('tas_wgrad(Tensor g, Tensor? mask, Tensor? gate, Tensor x, int stride, int window_length) -> Tensor')
def tas_wgrad(g, mask, gate, x, stride, window_length):
    """``[N L + N + 1]``: ``dW [N, L]``, ``sum_{b, tau} g [N]`` and ``sum x [1]`` (``ptmi_tas_wgrad``); ``g [B, N, E]``, ``x [B, T]`` or,
    with ``mask [K, B, N, E]``, ``[K, B, T]``."""
    lib = _lib.load()
    B, N, E = g.shape
    L = window_length
    K = 1 if mask is None else mask.shape[0]
    assert g.is_contiguous() and x.is_contiguous() and x.shape[:-1] == ((B,) if mask is None else (K, B)), (g.shape, x.shape)
    assert mask is None or (mask.shape == (K, B, N, E) and mask.is_contiguous())
    assert gate is None or (gate.shape == g.shape and gate.is_contiguous())
    ws = torch.empty(int(lib.ptmi_tas_wgrad_workspace_elems(B, N, L, stride, E)), dtype=torch.float32, device=g.device)
    out = torch.empty(N * L + N + 1, dtype=torch.float32, device=g.device)
    _lib.call('ptmi_tas_wgrad', g.data_ptr(), _lib.ptr(mask), _lib.ptr(gate), x.data_ptr(), K, B, x.shape[-1], N, L, stride, E,
              ws.data_ptr(), out.data_ptr(), _lib.stream(g.device), timer='tas_wgrad')
    return out


# ------------------------------------------------------------------------------------------------ Conv-TasNet block (channels last)
def _tcn_dims(x, channels_of=None):
    assert x.dim() == 3 and x.is_contiguous() and x.dtype == torch.float32, (x.shape, x.stride(), x.dtype)
    B, T, C = x.shape
    assert channels_of is None or channels_of.shape[0] == C, (x.shape, channels_of.shape)
    return B, T, C


def _doubles(n, device):
    return torch.empty(int(n), dtype=torch.float64, device=device)


@_register('tcn_depthwise_forward(Tensor u, Tensor slope_in, Tensor weight, Tensor? bias, Tensor slope_out, int dilation, float eps) '
           '-> (Tensor, Tensor)')
def tcn_depthwise_forward(u, slope_in, weight, bias, slope_out, dilation, eps):
    """``u [B, T, H]``, ``weight [H, (1,) K]`` -> ``(v [B, T, H], stats [B, 2])``: ``v = prelu(conv(pad(prelu(u))))`` and the per-example
    ``(mean, rstd)`` of ``v`` (``ptmi_tcn_depthwise_forward``)."""
    lib = _lib.load()
    B, T, H = _tcn_dims(u, weight)
    K = weight.numel() // H
    assert weight.is_contiguous() and slope_in.numel() == 1 and slope_out.numel() == 1 and (bias is None or bias.is_contiguous())
    v = torch.empty_like(u)
    stats = torch.empty((B, 2), dtype=torch.float32, device=u.device)
    ws = _doubles(lib.ptmi_tcn_depthwise_workspace_elems(B, T, H, K), u.device)
    _lib.call('ptmi_tcn_depthwise_forward', u.data_ptr(), slope_in.data_ptr(), weight.data_ptr(), _lib.ptr(bias), slope_out.data_ptr(),
              v.data_ptr(), stats.data_ptr(), ws.data_ptr(), B, T, H, K, dilation, eps, _lib.stream(u.device),
              timer='tcn_depthwise_forward')
    return v, stats


@_register('tcn_depthwise_backward(Tensor gv, Tensor u, Tensor slope_in, Tensor weight, Tensor? bias, Tensor slope_out, int dilation) '
           '-> (Tensor, Tensor)')
def tcn_depthwise_backward(gv, u, slope_in, weight, bias, slope_out, dilation):
    """``(gu [B, T, H], dparams [H K + H + 2])``: ``d weight | d bias | d slope_in | d slope_out`` (``ptmi_tcn_depthwise_backward``)."""
    lib = _lib.load()
    B, T, H = _tcn_dims(u, weight)
    K = weight.numel() // H
    assert gv.shape == u.shape and gv.is_contiguous() and weight.is_contiguous()
    gz, gu = torch.empty_like(u), torch.empty_like(u)
    dparams = torch.empty(H * K + H + 2, dtype=torch.float32, device=u.device)
    ws = _doubles(lib.ptmi_tcn_depthwise_workspace_elems(B, T, H, K), u.device)
    _lib.call('ptmi_tcn_depthwise_backward', gv.data_ptr(), u.data_ptr(), slope_in.data_ptr(), weight.data_ptr(), _lib.ptr(bias),
              slope_out.data_ptr(), gz.data_ptr(), gu.data_ptr(), dparams.data_ptr(), ws.data_ptr(), B, T, H, K, dilation,
              _lib.stream(u.device), timer='tcn_depthwise_backward')
    return gu, dparams


@_register('tcn_norm_stats(Tensor x, bool rows, float eps) -> Tensor')
def tcn_norm_stats(x, rows, eps):
    """``(mean, rstd)`` of ``x [B, T, C]`` per example ``[B, 2]`` or, ``rows``, per row ``[B T, 2]`` (``ptmi_tcn_norm_stats``)."""
    lib = _lib.load()
    B, T, C = _tcn_dims(x)
    stats = torch.empty((B * T if rows else B, 2), dtype=torch.float32, device=x.device)
    ws = None if rows else _doubles(lib.ptmi_tcn_norm_workspace_elems(B, T, C), x.device)
    _lib.call('ptmi_tcn_norm_stats', x.data_ptr(), stats.data_ptr(), _lib.ptr(ws), B, T, C, int(rows), eps, _lib.stream(x.device),
              timer='tcn_norm_stats')
    return stats


@_register('tcn_norm_apply(Tensor x, Tensor stats, Tensor gamma, Tensor beta, bool rows) -> Tensor')
def tcn_norm_apply(x, stats, gamma, beta, rows):
    """``gamma[c] (x - mean_g) rstd_g + beta[c]`` with ``stats [G, 2]`` from ``tcn_norm_stats`` / ``tcn_depthwise_forward``
    (``ptmi_tcn_norm_apply``)."""
    B, T, C = _tcn_dims(x)
    assert stats.shape == (B * T if rows else B, 2) and stats.is_contiguous() and stats.dtype == torch.float32, stats.shape
    assert gamma.numel() == C and beta.numel() == C and gamma.is_contiguous() and beta.is_contiguous()
    y = torch.empty_like(x)
    _lib.call('ptmi_tcn_norm_apply', x.data_ptr(), stats.data_ptr(), gamma.data_ptr(), beta.data_ptr(), y.data_ptr(), B, T, C, int(rows),
              _lib.stream(x.device), timer='tcn_norm_apply')
    return y


@_register('tcn_norm_backward(Tensor gy, Tensor x, Tensor stats, Tensor gamma, bool rows) -> (Tensor, Tensor)')
def tcn_norm_backward(gy, x, stats, gamma, rows):
    """``(dx [B, T, C], dparams [2 C])``: ``d gamma | d beta`` (``ptmi_tcn_norm_backward``)."""
    lib = _lib.load()
    B, T, C = _tcn_dims(x)
    assert gy.shape == x.shape and gy.is_contiguous() and gamma.numel() == C and gamma.is_contiguous()
    assert stats.shape == (B * T if rows else B, 2) and stats.is_contiguous(), stats.shape
    dx = torch.empty_like(x)
    dparams = torch.empty(2 * C, dtype=torch.float32, device=x.device)
    gsum = torch.empty_like(stats)
    ws = _doubles(lib.ptmi_tcn_norm_workspace_elems(B, T, C), x.device)
    _lib.call('ptmi_tcn_norm_backward', gy.data_ptr(), x.data_ptr(), stats.data_ptr(), gamma.data_ptr(), dx.data_ptr(), dparams.data_ptr(),
              gsum.data_ptr(), ws.data_ptr(), B, T, C, int(rows), _lib.stream(x.device), timer='tcn_norm_backward')
    return dx, dparams


# ------------------------------------------------------------------------------------------------ TasNet glue (csrc/tasnet.hip)
#: the activation codes of ptmi_tasnet_mask_head_*
TASNET_ACTIVATIONS = {'sigmoid': 0, 'relu': 1, 'leaky_relu': 2, 'elu': 3, 'tanh': 4, 'identity': 5}


def _f32c(*tensors):
    for t in tensors:
        assert t is None or (t.is_contiguous() and t.dtype == torch.float32), (t.shape, t.stride(), t.dtype)


def _lengths(lengths, B):
    if lengths is None:
        return None, 0
    assert lengths.dtype in (torch.int32, torch.int64) and lengths.shape == (B,) and lengths.is_contiguous() and lengths.is_cuda, \
        (lengths.dtype, lengths.shape, lengths.device)
    return lengths, int(lengths.dtype == torch.int64)


@_register('tasnet_entry_norm_forward(Tensor w, Tensor gamma, Tensor beta, Tensor? lengths, float eps) -> (Tensor, Tensor)')
def tasnet_entry_norm_forward(w, gamma, beta, lengths, eps):
    """``w [B, N, E]`` -> ``(y [B, E, N], stats [B E, 2])``: the layer norm over the channels of every frame below ``lengths[b]``,
    zeros from there on (``ptmi_tasnet_entry_norm_forward``)."""
    _f32c(w, gamma, beta)
    B, N, E = w.shape
    assert gamma.numel() == N and beta.numel() == N
    lengths, is64 = _lengths(lengths, B)
    y = torch.empty((B, E, N), dtype=torch.float32, device=w.device)
    stats = torch.empty((B * E, 2), dtype=torch.float32, device=w.device)
    _lib.call('ptmi_tasnet_entry_norm_forward', w.data_ptr(), gamma.data_ptr(), beta.data_ptr(), _lib.ptr(lengths), is64, y.data_ptr(),
              stats.data_ptr(), B, N, E, eps, _lib.stream(w.device), timer='tasnet_entry_norm_forward')
    return y, stats


@_register('tasnet_entry_norm_backward(Tensor gy, Tensor w, Tensor stats, Tensor gamma, Tensor? lengths) -> (Tensor, Tensor)')
def tasnet_entry_norm_backward(gy, w, stats, gamma, lengths):
    """``(dw [B, N, E], dparams [2 N])``: ``d gamma | d beta`` (``ptmi_tasnet_entry_norm_backward``)."""
    lib = _lib.load()
    _f32c(gy, w, stats, gamma)
    B, N, E = w.shape
    assert gy.shape == (B, E, N) and stats.shape == (B * E, 2) and gamma.numel() == N
    lengths, is64 = _lengths(lengths, B)
    dw = torch.empty_like(w)
    dparams = torch.empty(2 * N, dtype=torch.float32, device=w.device)
    ws = _doubles(lib.ptmi_tasnet_entry_norm_workspace_elems(B, N, E), w.device)
    _lib.call('ptmi_tasnet_entry_norm_backward', gy.data_ptr(), w.data_ptr(), stats.data_ptr(), gamma.data_ptr(), _lib.ptr(lengths), is64,
              dw.data_ptr(), dparams.data_ptr(), ws.data_ptr(), B, N, E, _lib.stream(w.device), timer='tasnet_entry_norm_backward')
    return dw, dparams


@_register('tasnet_prelu_forward(Tensor x, Tensor slope) -> Tensor')
def tasnet_prelu_forward(x, slope):
    """``x > 0 ? x : slope x`` with one slope in device memory (``ptmi_tasnet_prelu_forward``)."""
    _f32c(x, slope)
    assert slope.numel() == 1
    y = torch.empty_like(x)
    _lib.call('ptmi_tasnet_prelu_forward', x.data_ptr(), slope.data_ptr(), y.data_ptr(), x.numel(), _lib.stream(x.device),
              timer='tasnet_prelu_forward')
    return y


@_register('tasnet_prelu_backward(Tensor g, Tensor x, Tensor slope) -> (Tensor, Tensor)')
def tasnet_prelu_backward(g, x, slope):
    """``(gx, dslope [1])`` (``ptmi_tasnet_prelu_backward``)."""
    lib = _lib.load()
    _f32c(g, x, slope)
    assert g.shape == x.shape and slope.numel() == 1
    gx = torch.empty_like(x)
    dslope = torch.empty(1, dtype=torch.float32, device=x.device)
    ws = _doubles(lib.ptmi_tasnet_prelu_workspace_elems(x.numel()), x.device)
    _lib.call('ptmi_tasnet_prelu_backward', g.data_ptr(), x.data_ptr(), slope.data_ptr(), gx.data_ptr(), dslope.data_ptr(), ws.data_ptr(),
              x.numel(), _lib.stream(x.device), timer='tasnet_prelu_backward')
    return gx, dslope


@_register('tasnet_mask_head_forward(Tensor z, int K, int N, int A, int activation) -> (Tensor, Tensor)')
def tasnet_mask_head_forward(z, K, N, A, activation):
    """``z [B, E, A + K N]`` -> ``(m [K, B, N, E], additional [B, A, E])`` (``ptmi_tasnet_mask_head_forward``)."""
    _f32c(z)
    B, E, C = z.shape
    assert C == A + K * N, (z.shape, K, N, A)
    m = torch.empty((K, B, N, E), dtype=torch.float32, device=z.device)
    add = torch.empty((B, A, E), dtype=torch.float32, device=z.device)
    _lib.call('ptmi_tasnet_mask_head_forward', z.data_ptr(), m.data_ptr(), add.data_ptr() if A else None, B, E, N, K, A, activation,
              _lib.stream(z.device), timer='tasnet_mask_head_forward')
    return m, add


@_register('tasnet_mask_head_backward(Tensor gm, Tensor m, Tensor? g_additional, int A, int activation) -> Tensor')
def tasnet_mask_head_backward(gm, m, g_additional, A, activation):
    """``gz [B, E, A + K N]`` from the gradients of both outputs and the saved ``m`` (``ptmi_tasnet_mask_head_backward``)."""
    _f32c(gm, m, g_additional)
    K, B, N, E = m.shape
    assert gm.shape == m.shape and (g_additional is None or g_additional.shape == (B, A, E))
    gz = torch.empty((B, E, A + K * N), dtype=torch.float32, device=m.device)
    _lib.call('ptmi_tasnet_mask_head_backward', gm.data_ptr(), m.data_ptr(), _lib.ptr(g_additional) if A else None, gz.data_ptr(), B, E, N,
              K, A, activation, _lib.stream(m.device), timer='tasnet_mask_head_backward')
    return gz


@_register('tasnet_center(Tensor x, int K, int B, int T_in, int T_out, bool backward) -> Tensor')
def tasnet_center(x, K, B, T_in, T_out, backward):
    """``x [K, B, T_in]`` -> ``[B, K, T_out]`` with the mean over ``T_out`` taken off, or (``backward``) the adjoint ``[B, K, T_out]``
    -> ``[K, B, T_in]`` (``ptmi_tasnet_center``)."""
    lib = _lib.load()
    _f32c(x)
    assert x.shape == ((B, K, T_out) if backward else (K, B, T_in)), (x.shape, K, B, T_in, T_out, backward)
    out = torch.empty((K, B, T_in) if backward else (B, K, T_out), dtype=torch.float32, device=x.device)
    ws = _doubles(lib.ptmi_tasnet_center_workspace_elems(K, B, T_in, T_out), x.device)
    _lib.call('ptmi_tasnet_center', x.data_ptr(), out.data_ptr(), ws.data_ptr(), K, B, T_in, T_out, int(backward), _lib.stream(x.device),
              timer='tasnet_center')
    return out


# ------------------------------------------------------------------------------------------------ One-and-Rest PIT (csrc/orpit.hip)
def _rows(x):
    assert x.dim() == 3 and x.dtype == torch.float32 and (x.stride(2) == 1 or x.shape[2] == 1), (x.shape, x.stride(), x.dtype)
    return x


@_register('td_rect_stats(Tensor est, Tensor? tgt, bool want_gram) -> (Tensor, Tensor)')
def td_rect_stats(est, tgt, want_gram):
    """``est [B, M, T]``, ``tgt [B, K, T]`` (None: ``K = 0``; time contiguous, any batch / row strides) -> ``(stats [B, M K + M],
    gram [B, K, K])`` float64: ``sum e_m t_j | sum e_m^2`` and, ``want_gram``, ``sum t_j t_l`` (else empty) (``ptmi_td_rect_stats``)."""
    lib = _lib.load()
    B, M, T = _rows(est).shape
    K = 0 if tgt is None else _rows(tgt).shape[1]
    assert tgt is None or (tgt.shape[0], tgt.shape[2]) == (B, T), (est.shape, tgt.shape)
    stats = _doubles(B * (M * K + M), est.device).view(B, M * K + M)
    gram = _doubles(B * K * K if want_gram else 0, est.device).view(B if want_gram else 0, K, K)
    ws = _doubles(lib.ptmi_td_rect_workspace_elems(B, M, K, T), est.device)
    strides = _lib.int64s(est.stride(0), est.stride(1), *((tgt.stride(0), tgt.stride(1)) if K else (0, 0)))
    _lib.call('ptmi_td_rect_stats', est.data_ptr(), tgt.data_ptr() if K else None, B, M, K, T, strides, ws.data_ptr(), stats.data_ptr(),
              gram.data_ptr() if want_gram and K else None, _lib.stream(est.device), timer='td_rect_stats')
    return stats, gram


@_register('orpit_select(Tensor stats, Tensor gram, Tensor alive, int n) -> (Tensor, Tensor, Tensor, Tensor, Tensor)')
def orpit_select(stats, gram, alive, n):
    """One OR-PIT iteration from ``td_rect_stats`` (``M = 2``): ``(loss [B] fp32, choice [B] int32, alive_out [B, K] int32, coef_a [B, 2],
    coef_b [B, 2, K])`` (``ptmi_orpit_select``)."""
    B, K = alive.shape
    assert stats.shape == (B, 2 * K + 2) and stats.dtype == torch.float64 and stats.is_contiguous(), (stats.shape, stats.dtype)
    assert alive.dtype == torch.int32 and alive.is_contiguous(), (alive.dtype, alive.stride())
    assert K == 0 or (gram.shape == (B, K, K) and gram.dtype == torch.float64 and gram.is_contiguous()), (gram.shape, gram.dtype)
    dev = stats.device
    loss = torch.empty(B, dtype=torch.float32, device=dev)
    choice = torch.empty(B, dtype=torch.int32, device=dev)
    alive_out = torch.empty_like(alive)
    coef_a = torch.empty((B, 2), dtype=torch.float32, device=dev)
    coef_b = torch.empty((B, 2, K), dtype=torch.float32, device=dev)
    none = (lambda t: t.data_ptr() if K else None)
    _lib.call('ptmi_orpit_select', stats.data_ptr(), none(gram), none(alive), none(alive_out), loss.data_ptr(), choice.data_ptr(),
              coef_a.data_ptr(), none(coef_b), B, K, n, _lib.stream(dev), timer='orpit_select')
    return loss, choice, alive_out, coef_a, coef_b


@_register('td_rect_lincomb(Tensor est, Tensor? tgt, Tensor? g, Tensor coef_a, Tensor coef_b) -> Tensor')
def td_rect_lincomb(est, tgt, g, coef_a, coef_b):
    """``out[b, m] = g[b] (coef_a[b, m] est[b, m] + sum_j coef_b[b, m, j] tgt[b, j])`` as a contiguous ``[B, M, T]``
    (``ptmi_td_rect_lincomb``)."""
    B, M, T = _rows(est).shape
    K = 0 if tgt is None else _rows(tgt).shape[1]
    _f32c(g, coef_a, coef_b)
    assert coef_a.shape == (B, M) and coef_b.shape == (B, M, K) and (g is None or g.shape == (B,)), (coef_a.shape, coef_b.shape)
    out = torch.empty((B, M, T), dtype=torch.float32, device=est.device)
    strides = _lib.int64s(est.stride(0), est.stride(1), *((tgt.stride(0), tgt.stride(1)) if K else (0, 0)), out.stride(0), out.stride(1))
    _lib.call('ptmi_td_rect_lincomb', est.data_ptr(), tgt.data_ptr() if K else None, _lib.ptr(g), coef_a.data_ptr(),
              coef_b.data_ptr() if K else None, B, M, K, T, strides, out.data_ptr(), _lib.stream(est.device), timer='td_rect_lincomb')
    return out


def _flag_dims(additional, weight, bias, mask, encoded, k):
    _f32c(additional, weight, bias, mask, encoded)
    B, A, E = additional.shape
    assert weight.numel() == A and (bias is None or bias.numel() == 1) and A >= 1, (additional.shape, weight.shape)
    K = N = 0
    if mask is not None:
        K, _, N, _ = mask.shape
        assert mask.shape == (K, B, N, E) and 0 <= k < K and (encoded is None or encoded.shape == (B, N, E)), \
            (mask.shape, additional.shape, k, None if encoded is None else encoded.shape)
    else:
        assert encoded is None
    return B, A, E, N, K


@_register('orpit_flag_forward(Tensor additional, Tensor weight, Tensor bias, Tensor? mask, Tensor? encoded, int k) '
           '-> (Tensor, Tensor, Tensor, Tensor)')
def orpit_flag_forward(additional, weight, bias, mask, encoded, k):
    """``(pre [B, E], flag [B], w [B, E] (empty without mask), stat [B, 2] float64)``; a ``mask [K, B, N, E]`` selects the weighted mean
    with ``w = mean_n (mask[k] encoded)^2`` (``ptmi_orpit_flag_forward``)."""
    lib = _lib.load()
    B, A, E, N, K = _flag_dims(additional, weight, bias, mask, encoded, k)
    dev = additional.device
    pre = torch.empty((B, E), dtype=torch.float32, device=dev)
    w = torch.empty((B, E) if K else (0,), dtype=torch.float32, device=dev)
    flag = torch.empty(B, dtype=torch.float32, device=dev)
    stat = _doubles(2 * B, dev).view(B, 2)
    ws = _doubles(lib.ptmi_orpit_flag_workspace_elems(B, A, E), dev)
    _lib.call('ptmi_orpit_flag_forward', additional.data_ptr(), weight.data_ptr(), bias.data_ptr(), _lib.ptr(mask), _lib.ptr(encoded),
              pre.data_ptr(), w.data_ptr() if K else None, flag.data_ptr(), stat.data_ptr(), ws.data_ptr(), B, A, E, N, K, k, int(K > 0),
              _lib.stream(dev), timer='orpit_flag_forward')
    return pre, flag, w, stat


@_register('orpit_flag_backward(Tensor gflag, Tensor? gpre, Tensor flag, Tensor stat, Tensor pre, Tensor w, Tensor additional, '
           'Tensor weight, Tensor? mask, Tensor? encoded, int k) -> (Tensor, Tensor, Tensor?, Tensor?)')
def orpit_flag_backward(gflag, gpre, flag, stat, pre, w, additional, weight, mask, encoded, k):
    """``(d additional, dparams [A + 1] = d weight | d bias, d mask or None, d encoded or None)`` (``ptmi_orpit_flag_backward``)."""
    lib = _lib.load()
    B, A, E, N, K = _flag_dims(additional, weight, None, mask, encoded, k)
    _f32c(gflag, gpre, flag, pre, w)
    assert gflag.shape == (B,) and (gpre is None or gpre.shape == (B, E)) and pre.shape == (B, E) and stat.shape == (B, 2)
    dev = additional.device
    dadd = torch.empty_like(additional)
    dparams = torch.empty(A + 1, dtype=torch.float32, device=dev)
    dmask = torch.empty_like(mask) if K else None
    denc = torch.empty_like(encoded) if encoded is not None else None
    ws = _doubles(lib.ptmi_orpit_flag_workspace_elems(B, A, E), dev)
    _lib.call('ptmi_orpit_flag_backward', gflag.data_ptr(), _lib.ptr(gpre), flag.data_ptr(), stat.data_ptr(), pre.data_ptr(),
              w.data_ptr() if K else None, additional.data_ptr(), weight.data_ptr(), _lib.ptr(mask), _lib.ptr(encoded), dadd.data_ptr(),
              dparams.data_ptr(), _lib.ptr(dmask), _lib.ptr(denc), ws.data_ptr(), B, A, E, N, K, k, int(K > 0), _lib.stream(dev),
              timer='orpit_flag_backward')
    return dadd, dparams, dmask, denc


# ------------------------------------------------------------------------------------------------ mask loss (csrc/mask_loss.hip)
def _mask_loss_args(logits, target, power, num_frames):
    """``(B, C, T, F, power kind, the HOST stride array)`` of ``[B, C, T, F]`` operands with unit stride on ``F``."""
    assert logits.dim() == 4 and logits.shape == target.shape and logits.dtype == target.dtype == torch.float32, \
        (logits.shape, target.shape, logits.dtype, target.dtype)
    B, C, T, F = logits.shape
    kind = 0
    if power is not None:
        assert power.shape == logits.shape and power.dtype in (torch.float32, torch.complex64), (power.shape, power.dtype)
        kind = 2 if power.dtype == torch.complex64 else 1
    for t in (logits, target, power):
        assert t is None or F == 1 or t.stride(3) == 1, t.stride()
    assert num_frames is None or (num_frames.dtype == torch.int32 and num_frames.shape == (B,) and num_frames.is_contiguous()), \
        (num_frames.dtype, num_frames.shape)
    strides = _lib.int64s(*logits.stride()[:3], *target.stride()[:3], *(power.stride()[:3] if kind else (0, 0, 0)))
    return B, C, T, F, kind, strides


@_register('mask_loss_forward(Tensor logits, Tensor target, Tensor? power, Tensor? num_frames, int reduction) '
           '-> (Tensor, Tensor?, Tensor, Tensor)')
def mask_loss_forward(logits, target, power, num_frames, reduction):
    """``(pooled [B], weighted [B] or None, stat [B, 4] float64, sel [B, 2] int32)`` of ``logits, target [B, C, T, F]`` (strided, unit
    stride on ``F``), ``power`` float32 or complex64, ``num_frames`` int32 ``[B]``; ``reduction`` 0 mean, 1 median, 2 min, 3 max
    (``ptmi_mask_loss_forward``)."""
    lib = _lib.load()
    B, C, T, F, kind, strides = _mask_loss_args(logits, target, power, num_frames)
    dev = logits.device
    pooled = torch.empty(B, dtype=torch.float32, device=dev)
    weighted = torch.empty(B, dtype=torch.float32, device=dev) if kind else None
    stat = _doubles(4 * B, dev).view(B, 4)
    sel = torch.empty((B, 2), dtype=torch.int32, device=dev)
    ws = _doubles(lib.ptmi_mask_loss_workspace_elems(B, C, T, F), dev)
    _lib.call('ptmi_mask_loss_forward', logits.data_ptr(), target.data_ptr(), _lib.ptr(power), kind, _lib.ptr(num_frames), strides, B, C, T,
              F, reduction, ws.data_ptr(), pooled.data_ptr(), _lib.ptr(weighted), stat.data_ptr(), sel.data_ptr(), _lib.stream(dev),
              timer='mask_loss_forward')
    return pooled, weighted, stat, sel


@_register('mask_loss_backward(Tensor logits, Tensor target, Tensor? power, Tensor? num_frames, Tensor? g_pooled, Tensor? g_weighted, '
           'Tensor stat, Tensor sel, int reduction) -> Tensor')
def mask_loss_backward(logits, target, power, num_frames, g_pooled, g_weighted, stat, sel, reduction):
    """``d logits [B, C, T, F]`` (dense) from ``g_pooled`` / ``g_weighted [B]`` (either may be None) (``ptmi_mask_loss_backward``)."""
    B, C, T, F, kind, strides = _mask_loss_args(logits, target, power, num_frames)
    _f32c(g_pooled, g_weighted)
    assert (g_pooled is None or g_pooled.shape == (B,)) and (g_weighted is None or g_weighted.shape == (B,))
    assert stat.shape == (B, 4) and stat.dtype == torch.float64 and sel.shape == (B, 2) and sel.dtype == torch.int32
    dev = logits.device
    out = torch.empty((B, C, T, F), dtype=torch.float32, device=dev)
    _lib.call('ptmi_mask_loss_backward', logits.data_ptr(), target.data_ptr(), _lib.ptr(power), kind, _lib.ptr(num_frames), strides,
              _lib.ptr(g_pooled), _lib.ptr(g_weighted), stat.data_ptr(), sel.data_ptr(), B, C, T, F, reduction, out.data_ptr(),
              _lib.stream(dev), timer='mask_loss_backward')
    return out


# ------------------------------------------------------------------------------------------------ beamforming (csrc/beamform.hip)
def _bf_spectrum(x):
    """``[B, C, T, F]`` complex64, contiguous -> its ``(B, C, T, F)``."""
    assert x.dim() == 4 and x.dtype == torch.complex64 and x.is_contiguous(), (x.shape, x.stride(), x.dtype)
    return x.shape


def _bf_frames(frames, B):
    assert frames is None or (frames.dtype == torch.int32 and frames.shape == (B,) and frames.is_contiguous()), \
        (frames.dtype, frames.shape)
    return _lib.ptr(frames)


@_register('bf_psd(Tensor observation, Tensor? mask0, Tensor? mask1, Tensor? frames, bool normalize) -> Tensor')
def bf_psd(observation, mask0, mask1, frames, normalize):
    """``observation [B, C, T, F]`` complex64 and up to two masks (``[B, C, T, F]``: the channel median is taken in the kernel,
    ``[B, T, F]``: as it is; none: the plain covariance) -> ``psd [M, B, F, C, C]`` complex128, one pass over the observation
    (``ptmi_bf_psd``)."""
    lib = _lib.load()
    B, C, T, F = _bf_spectrum(observation)
    masks = [m for m in (mask0, mask1) if m is not None]
    assert mask0 is not None or mask1 is None
    _f32c(*masks)
    mode = 0 if not masks else masks[0].dim() - 2
    assert all(tuple(m.shape) == ((B, C, T, F) if mode == 2 else (B, T, F)) for m in masks), ([m.shape for m in masks], observation.shape)
    M = max(len(masks), 1)
    dev = observation.device
    psd = _doubles(M * B * F * C * C * 2, dev).view(M, B, F, C, C, 2)
    ws = _doubles(lib.ptmi_bf_psd_workspace_elems(B, C, T, F, M), dev)
    _lib.call('ptmi_bf_psd', observation.data_ptr(), _lib.ptr(mask0), _lib.ptr(mask1), _bf_frames(frames, B), B, C, T, F, M, mode,
              int(normalize), ws.data_ptr(), psd.data_ptr(), _lib.stream(dev), timer='bf_psd')
    return torch.view_as_complex(psd)


@_register('bf_souden(Tensor target_psd, Tensor noise_psd, int ref_channel) -> (Tensor, Tensor, Tensor)')
def bf_souden(target_psd, noise_psd, ref_channel):
    """``[B, F, C, C]`` complex128 PSD matrices -> ``(w [B, F, C] complex64, w_all [B, F, C, C] complex64, ref [B] int32)``;
    ``ref_channel < 0``: the reference channel is chosen on the device (``ptmi_bf_souden``)."""
    for p in (target_psd, noise_psd):
        assert p.dim() == 4 and p.dtype == torch.complex128 and p.is_contiguous() and p.shape == target_psd.shape, (p.shape, p.dtype)
    B, F, C, _ = target_psd.shape
    assert target_psd.shape[3] == C and ref_channel < C, (target_psd.shape, ref_channel)
    dev = target_psd.device
    w_all = torch.empty((B, F, C, C), dtype=torch.complex64, device=dev)
    w = torch.empty((B, F, C), dtype=torch.complex64, device=dev)
    ref = torch.empty(B, dtype=torch.int32, device=dev)
    numden = _doubles(B * F * C * 2 if ref_channel < 0 else 0, dev)
    _lib.call('ptmi_bf_souden', target_psd.data_ptr(), noise_psd.data_ptr(), B, F, C, max(int(ref_channel), -1), w_all.data_ptr(),
              numden.data_ptr() if ref_channel < 0 else None, w.data_ptr(), ref.data_ptr(), _lib.stream(dev), timer='bf_souden')
    return w, w_all, ref


@_register('bf_apply(Tensor vector, Tensor mix, Tensor? frames) -> Tensor')
def bf_apply(vector, mix, frames):
    """``vector [B, F, C]``, ``mix [B, C, T, F]`` complex64 -> ``[B, T, F]``: ``sum_c conj(vector) mix`` (``ptmi_bf_apply``)."""
    B, C, T, F = _bf_spectrum(mix)
    assert vector.shape == (B, F, C) and vector.dtype == torch.complex64 and vector.is_contiguous(), (vector.shape, vector.dtype)
    out = torch.empty((B, T, F), dtype=torch.complex64, device=mix.device)
    _lib.call('ptmi_bf_apply', vector.data_ptr(), mix.data_ptr(), _bf_frames(frames, B), B, C, T, F, out.data_ptr(),
              _lib.stream(mix.device), timer='bf_apply')
    return out


def _bf_vector(vector):
    """``[B, F, C]`` complex64, contiguous -> its ``(B, F, C)``."""
    assert vector.dim() == 3 and vector.dtype == torch.complex64 and vector.is_contiguous(), (vector.shape, vector.dtype)
    return vector.shape


@_register('bf_eig(Tensor target_psd, Tensor? noise_psd, bool gev, bool ban) -> (Tensor, Tensor, Tensor)')
def bf_eig(target_psd, noise_psd, gev, ban):
    """``[B, F, C, C]`` complex128 PSD matrices -> ``(w [B, F, C] complex64, lambda [B, F] float64, sweeps [B, F] int32)``: the
    principal generalized eigenvector of ``(target, noise)`` (``gev``) or the principal eigenvector of ``target``, blind analytic
    normalization with ``noise`` included when ``ban`` (``ptmi_bf_eig``)."""
    assert noise_psd is not None or not (gev or ban)
    for p in (target_psd, noise_psd):
        assert p is None or (p.dim() == 4 and p.dtype == torch.complex128 and p.is_contiguous() and p.shape == target_psd.shape), \
            (p.shape, p.dtype)
    B, F, C, _ = target_psd.shape
    assert target_psd.shape[3] == C, target_psd.shape
    dev = target_psd.device
    w = torch.empty((B, F, C), dtype=torch.complex64, device=dev)
    lam = torch.empty((B, F), dtype=torch.float64, device=dev)
    sweeps = torch.empty((B, F), dtype=torch.int32, device=dev)
    _lib.call('ptmi_bf_eig', target_psd.data_ptr(), _lib.ptr(noise_psd), B, F, C, 0 if gev else 1, int(ban), w.data_ptr(), lam.data_ptr(),
              sweeps.data_ptr(), _lib.stream(dev), timer='bf_eig')
    return w, lam, sweeps


@_register('bf_ban(Tensor vector, Tensor noise_psd) -> Tensor')
def bf_ban(vector, noise_psd):
    """``vector [B, F, C]`` complex64, ``noise_psd [B, F, C, C]`` complex128 -> the blind analytic normalization of the vector
    (``ptmi_bf_ban``)."""
    B, F, C = _bf_vector(vector)
    assert noise_psd.shape == (B, F, C, C) and noise_psd.dtype == torch.complex128 and noise_psd.is_contiguous(), \
        (noise_psd.shape, noise_psd.dtype)
    out = torch.empty_like(vector)
    _lib.call('ptmi_bf_ban', vector.data_ptr(), noise_psd.data_ptr(), B, F, C, out.data_ptr(), _lib.stream(vector.device), timer='bf_ban')
    return out


@_register('bf_phase(Tensor vector) -> Tensor')
def bf_phase(vector):
    """``vector [B, F, C]`` complex64 -> the vector with the phase of every bin aligned to the bin before it (``ptmi_bf_phase``)."""
    B, F, C = _bf_vector(vector)
    out = torch.empty_like(vector)
    _lib.call('ptmi_bf_phase', vector.data_ptr(), B, F, C, out.data_ptr(), _lib.stream(vector.device), timer='bf_phase')
    return out


# ------------------------------------------------------------------------------------------------ dense layers
_ZERO_WORDS = {}


def _zero_word(device):
    """One int32 word that is zero on the current stream: words of a buffer zeroed ONCE (a fill launch per 256 words instead of a
    zeroing launch in front of every reduction: five per training step); a buffer per stream, each word handed out once."""
    from . import capture as _capture
    if _capture.ACTIVE:                 # a captured step: words the graph itself zeroes at every replay
        return _capture.zero_word(device, 256)
    key = (device.index, torch.cuda.current_stream(device).cuda_stream)
    pool = _ZERO_WORDS.get(key)
    if pool is None or pool[1] >= pool[0].numel():
        if len(_ZERO_WORDS) > 16:
            _ZERO_WORDS.clear()
        pool = _ZERO_WORDS[key] = [torch.zeros(256, dtype=torch.int32, device=device), 0]
    pool[1] += 1
    return pool[0][pool[1] - 1:pool[1]]


@_register('absmax(Tensor x, int rows, int cols, int ld) -> Tensor')
def absmax(x, rows, cols, ld):
    out = _zero_word(x.device)
    _lib.call('ptmi_absmax_accumulate', x.data_ptr(), rows, cols, ld, out.data_ptr(), _lib.stream(x.device))
    return out


def _lstm_backward_persistent(gates, c, c0, dhy, w_hh_t, dg, dg_t, scratch, dc_carry, bs_dev, offs_dev, T, max_batch, rows, H, ndir,
                              s_begin, s_end, prefilled, step_masks=None, dc_n=None):
    """The one call of ``ptmi_lstm_backward_persistent`` (include/ptmi.h has its contract).  False: the configuration cannot be kept
    resident, or the call does not support the combination of arguments - nothing was enqueued, the caller takes another route;
    every other refusal raises."""
    return 0 == _lib.call('ptmi_lstm_backward_persistent', gates.data_ptr(), c.data_ptr(), _lib.ptr(c0), dhy.data_ptr(), _lib.ptr(dc_n),
                          w_hh_t.data_ptr(), _lib.ptr(dg), _lib.ptr(dg_t), bs_dev.data_ptr(), offs_dev.data_ptr(), _lib.ptr(step_masks),
                          scratch.data_ptr(), _lib.ptr(dc_carry), T, max_batch, rows, H, ndir, s_begin, s_end, int(prefilled),
                          _lib.stream(gates.device), timer='lstm_backward', accept=(-2,))


@_register('lstm_recurrence_backward_range(Tensor gates, Tensor c, Tensor? c0, Tensor dhy, Tensor w_hh_t, Tensor(a!) dg, '
           'Tensor(b!) scratch, Tensor(c!) dc_carry, Tensor bs_dev, Tensor offs_dev, int T, int max_batch, int rows, int H, '
           'int ndir, int s_begin, int s_end, int prefilled=0, Tensor? dc_n=None) -> bool')
def lstm_recurrence_backward_range(gates, c, c0, dhy, w_hh_t, dg, scratch, dc_carry, bs_dev, offs_dev, T, max_batch, rows, H, ndir,
                                   s_begin, s_end, prefilled=0, dc_n=None):
    """The persistent backward recurrence over the processing steps [s_begin, s_end) (ranges in order, same ``dg`` / ``scratch`` /
    ``dc_carry``); ``dc_n`` [ndir, max_batch, H]: + the gradient w.r.t. the final cell state (whole recurrence only).  False: the
    launch cannot be resident (nothing was run)."""
    assert dc_n is None or (dc_n.shape == (ndir, max_batch, H) and dc_n.is_contiguous()), dc_n.shape
    return _lstm_backward_persistent(gates, c, c0, dhy, w_hh_t, dg, None, scratch, dc_carry, bs_dev, offs_dev, T, max_batch, rows, H, ndir,
                                     s_begin, s_end, prefilled, dc_n=dc_n)


@_register('lstm_recurrence_backward_planes(Tensor gates, Tensor c, Tensor? c0, Tensor dhy, Tensor w_hh_t, Tensor(a!)? dg, '
           'Tensor(b!) dg_t, Tensor(c!) scratch, Tensor(d!)? dc_carry, Tensor bs_dev, Tensor offs_dev, int T, int max_batch, int rows, '
           'int H, int ndir, int s_begin, int s_end, int prefilled=0, Tensor? step_masks=None) -> bool')
def lstm_recurrence_backward_planes(gates, c, c0, dhy, w_hh_t, dg, dg_t, scratch, dc_carry, bs_dev, offs_dev, T, max_batch, rows, H, ndir,
                                    s_begin, s_end, prefilled=0, step_masks=None):
    """The persistent backward recurrence over the processing steps [s_begin, s_end) with the gate gradients leaving as bf16 planes
    of ``dgates^T`` (``dg_t``: ``ndir * ptmi_planes_elems(4H, range rows)`` bf16 values, the operand of the weight-gradient GEMMs)
    and, only when ``dg`` is given, as the row-major fp32 tensor too; ``step_masks``: a row-slot batch (whole recurrence, no initial
    states).  False: the launch cannot be resident (nothing was run)."""
    need = ndir * int(_lib.load().ptmi_planes_elems(4 * H, (s_end - s_begin) * max_batch))       # this step range's rows
    assert dg_t.dtype == torch.bfloat16 and dg_t.numel() >= need, (dg_t.dtype, dg_t.numel(), need)
    return _lstm_backward_persistent(gates, c, c0, dhy, w_hh_t, dg, dg_t, scratch, dc_carry, bs_dev, offs_dev, T, max_batch, rows, H, ndir,
                                     s_begin, s_end, prefilled, step_masks=step_masks)


@_register('lstm_bias_grad_add_(Tensor db, Tensor(a!)[] bias_ih_grad, Tensor(b!)[] bias_hh_grad) -> ()')
def lstm_bias_grad_add_(db, bias_ih_grad, bias_hh_grad):
    """``bias_ih_grad[d] += db[d]; bias_hh_grad[d] += db[d]`` for every direction in one launch (``ptmi_lstm_bias_grad_add``)."""
    ndir = len(bias_ih_grad)
    n = bias_ih_grad[0].numel()
    assert db.numel() == ndir * n and db.dtype == torch.float32 and db.is_contiguous()
    assert all(t.is_contiguous() and t.numel() == n and t.dtype == torch.float32 for t in list(bias_ih_grad) + list(bias_hh_grad))
    ih = (ctypes.c_void_p * ndir)(*[t.data_ptr() for t in bias_ih_grad])
    hh = (ctypes.c_void_p * ndir)(*[t.data_ptr() for t in bias_hh_grad])
    _lib.call('ptmi_lstm_bias_grad_add', db.data_ptr(), ndir, n, ih, hh, _lib.stream(db.device))


# ------------------------------------------------------------------------------------------------ LSTM parameter forms
@_register('lstm_weight_prep(Tensor[] w_ih, Tensor[] w_hh, Tensor[] b_ih, Tensor[] b_hh, int KP) -> '
           '(Tensor, Tensor, Tensor, Tensor, Tensor)')
def lstm_weight_prep(w_ih, w_hh, b_ih, b_hh, KP):
    ndir, (G, I), H = len(w_ih), w_ih[0].shape, w_hh[0].shape[1]
    dev = w_ih[0].device
    Ipad = (I + 3) // 4 * 4
    f32 = dict(dtype=torch.float32, device=dev)
    w_ih_cat, bias = torch.empty((ndir * G, Ipad), **f32), torch.empty(ndir * G, **f32)
    w_pad, w_t = torch.empty((ndir, G, KP), **f32), torch.empty((ndir, H, G), **f32)
    amax = torch.empty(2, dtype=torch.int32, device=dev)
    ptrs = [(ctypes.c_void_p * ndir)(*[t.data_ptr() for t in ts]) for ts in (w_ih, w_hh, b_ih, b_hh)]
    _lib.call('ptmi_lstm_weight_prep', *ptrs, ndir, H, I, w_ih_cat.data_ptr(), Ipad, bias.data_ptr(), w_pad.data_ptr(), KP, w_t.data_ptr(),
              amax.data_ptr(), _lib.stream(dev), timer='lstm_weight_prep')
    return w_ih_cat, bias, w_pad, w_t, amax


# ------------------------------------------------------------------------------------------------ optimizer step
@_register('grad_norm(Tensor flat) -> Tensor')
def grad_norm(flat):
    lib = _lib.load()
    ws = torch.empty(int(lib.ptmi_grad_norm_workspace_elems()), dtype=torch.float64, device=flat.device)
    out = torch.empty((), dtype=torch.float32, device=flat.device)
    _lib.call('ptmi_grad_norm', flat.data_ptr(), flat.numel(), ws.data_ptr(), out.data_ptr(), _lib.stream(flat.device), timer='grad_norm')
    return out


@_register('adam_flat_(Tensor(a!) flat_grad, Tensor(b!) exp_avg, Tensor(c!) exp_avg_sq, Tensor segments, Tensor(d!)[] params, '
           'Tensor? norm, float max_norm, Tensor? found_inf, Tensor? finite, Tensor step, float lr, float beta1, float beta2, '
           'float eps, float weight_decay, bool zero_grad, Tensor? hyper=None) -> Tensor')
def adam_flat_(flat_grad, exp_avg, exp_avg_sq, segments, params, norm, max_norm, found_inf, finite, step, lr, beta1, beta2, eps,
               weight_decay, zero_grad, hyper=None):
    # `params` are the tensors the segment table points into (listed so that the dispatcher sees what is written);
    # returns the 0-dim fp32 "applied" flag (0: the update was skipped)
    # `hyper`: device fp64 [6] (lr, beta1, beta2, eps, weight_decay, max_norm) that the kernel reads INSTEAD of the float arguments
    if hyper is not None:
        assert hyper.dtype == torch.float64 and hyper.numel() >= 6 and hyper.device == flat_grad.device and hyper.is_contiguous(), hyper
    applied = torch.empty((), dtype=torch.float32, device=flat_grad.device)
    _lib.call('ptmi_adam_flat', flat_grad.data_ptr(), exp_avg.data_ptr(), exp_avg_sq.data_ptr(), segments.data_ptr(), segments.shape[0],
              flat_grad.numel(), _lib.ptr(norm), max_norm, _lib.ptr(found_inf), _lib.ptr(finite), applied.data_ptr(), step.data_ptr(), lr,
              beta1, beta2, eps, weight_decay, _lib.ptr(hyper), int(zero_grad), _lib.stream(flat_grad.device), timer='adam_flat')
    return applied


# ------------------------------------------------------------------------------------------------ GEMM on split planes
@_register('pack_planes_t(Tensor x, Tensor? amax) -> Tensor')
def pack_planes_t(x, amax):
    """x [k, c] (fp32, unit inner stride) -> fp16 (hi, lo) planes of the c x k operand (``ptmi_pack_planes_t``)."""
    lib = _lib.load()
    k, c = x.shape
    out = torch.empty(int(lib.ptmi_planes_elems(c, k)), dtype=torch.float16, device=x.device)
    _lib.call('ptmi_pack_planes_t', x.data_ptr(), k, c, _ld(x), _lib.ptr(amax), out.data_ptr(), _lib.stream(x.device),
              timer=f'pack_planes_t:{k}x{c}')
    return out


@_register('pack_planes_n(Tensor x, Tensor? amax) -> Tensor')
def pack_planes_n(x, amax):
    """x [r, k] (fp32, unit inner stride) -> fp16 (hi, lo) planes of the r x k operand (``ptmi_pack_planes_n``)."""
    lib = _lib.load()
    r, k = x.shape
    out = torch.empty(int(lib.ptmi_planes_elems(r, k)), dtype=torch.float16, device=x.device)
    _lib.call('ptmi_pack_planes_n', x.data_ptr(), r, k, _ld(x), _lib.ptr(amax), out.data_ptr(), _lib.stream(x.device),
              timer=f'pack_planes_n:{r}x{k}')
    return out


@_register('gemm_planes_(Tensor(a!) out, Tensor a, Tensor? amax_a, Tensor b, Tensor? amax_b, Tensor? bias, int M, int N, int K, '
           'bool accumulate, int split_k) -> ()')
def gemm_planes_(out, a, amax_a, b, amax_b, bias, M, N, K, accumulate, split_k):
    _gemm_planes_call('ptmi_gemm_planes', 'gemm_planes', out, M, N, K, split_k,
                      (a.data_ptr(), _lib.ptr(amax_a), b.data_ptr(), _lib.ptr(amax_b), _lib.ptr(bias), out.data_ptr(), max(out.stride(0), N),
                       M, N, K, int(accumulate)))


@_register('gemm_planes_relu_(Tensor(a!) out, Tensor a, Tensor? amax_a, Tensor b, Tensor? amax_b, Tensor? bias, int M, int N, int K, '
           'int split_k, Tensor(b!) amax_out) -> ()')
def gemm_planes_relu_(out, a, amax_a, b, amax_b, bias, M, N, K, split_k, amax_out):
    """``out = relu(A B^T + bias)`` and the float bits of ``max out`` into the ZEROED word ``amax_out`` (``ptmi_gemm_planes_relu``)."""
    _gemm_planes_call('ptmi_gemm_planes_relu', 'gemm_planes', out, M, N, K, split_k,
                      (a.data_ptr(), _lib.ptr(amax_a), b.data_ptr(), _lib.ptr(amax_b), _lib.ptr(bias), out.data_ptr(), max(out.stride(0), N),
                       M, N, K), (amax_out.data_ptr(), 1))


@_register('relu_backward_absmax(Tensor g, Tensor y, Tensor(a!) amax_out) -> Tensor')
def relu_backward_absmax(g, y, amax_out):
    """``g`` where ``y > 0`` (``y``: the ReLU's output) else 0, and the float bits of its ``max |.|`` into the ZEROED word ``amax_out``."""
    assert g.dim() == 2 and g.shape == y.shape and g.stride(1) == 1 and y.stride(1) == 1
    out = torch.empty((g.shape[0], g.shape[1]), dtype=torch.float32, device=g.device)
    _lib.call('ptmi_relu_backward_absmax', g.data_ptr(), y.data_ptr(), out.data_ptr(), g.shape[0], g.shape[1], _ld(g), _ld(y), _ld(out),
              amax_out.data_ptr(), 1, _lib.stream(g.device), timer=f'relu_backward_absmax:{g.shape[0]}x{g.shape[1]}')
    return out


def _ld(x):
    """Row stride of a 2-D source with unit inner stride (a single row has none to speak of)."""
    return x.stride(0) if x.shape[0] > 1 else max(x.stride(0), x.shape[1])


def _products():
    """3 (fp32-equivalent) or 1 (the hi planes only: ``ops.gemm.PRODUCTS``, the reduced-precision reporting mode)."""
    from . import gemm
    return 1 if gemm.PRODUCTS == 1 else 3


def _gemm_planes_call(entry, timer, out, M, N, K, split_k, head, tail=()):
    """One single-product planes GEMM ``entry(*head, split_k, products, workspace, *tail, stream)``: the slab workspace ``split_k`` asks
    for, the timed call (``timer:MxNxK:split_k`` - ``bench.py`` parses the name) and its return code."""
    lib = _lib.load()
    nws = int(lib.ptmi_gemm_planes_workspace_elems(M, N, K, split_k))
    ws = torch.empty(nws, dtype=torch.float32, device=out.device) if nws else None
    _lib.call(entry, *head, split_k, _products(), _lib.ptr(ws), *tail, _lib.stream(out.device), timer=f'{timer}:{M}x{N}x{K}:{split_k}')


@_register('pack_planes_bf16(Tensor x, bool transposed) -> Tensor')
def pack_planes_bf16(x, transposed):
    """bf16 (hi, lo) planes, no scale (``ptmi_pack_planes_t_bf16`` / ``_n_bf16``): ``transposed`` - x [k, c], the operand's
    rows are x's columns; else x [r, k]."""
    lib = _lib.load()
    a, b = x.shape
    rows, k = (b, a) if transposed else (a, b)
    out = torch.empty(int(lib.ptmi_planes_elems(rows, k)), dtype=torch.bfloat16, device=x.device)
    _lib.call('ptmi_pack_planes_t_bf16' if transposed else 'ptmi_pack_planes_n_bf16', x.data_ptr(), a, b, _ld(x), out.data_ptr(),
              _lib.stream(x.device), timer=f'pack_planes_bf16:{a}x{b}')
    return out


@_register('pack_planes_into_(Tensor(a!) out, Tensor x, Tensor? amax, bool transposed, int kb_total, int kb_offset, int kb_count) -> ()')
def pack_planes_into_(out, x, amax, transposed, kb_total, kb_offset, kb_count):
    """A pack pass writing ``kb_count`` k blocks at k block ``kb_offset`` of planes ``out`` that have ``kb_total`` k blocks per row
    tile (``ptmi_pack_planes_into``); fp16 or bf16 by ``out.dtype``; ``x [r, k]``, or ``[k, c]`` when ``transposed``."""
    a, b = x.shape
    rows = b if transposed else a
    assert out.dtype in (torch.float16, torch.bfloat16) and out.numel() >= (rows + 15) // 16 * kb_total * 1024, (out.dtype, out.numel())
    _lib.call('ptmi_pack_planes_into', x.data_ptr(), a, b, _ld(x), int(transposed), int(out.dtype == torch.bfloat16), _lib.ptr(amax),
              out.data_ptr(), kb_total, kb_offset, kb_count, _lib.stream(x.device), timer=f'pack_planes_into:{a}x{b}')


@_register('gemm_planes_bf16_(Tensor(a!) out, Tensor a, int a_offset, Tensor b, Tensor? bias, int M, int N, int K, bool accumulate, '
           'int split_k) -> ()')
def gemm_planes_bf16_(out, a, a_offset, b, bias, M, N, K, accumulate, split_k):
    """``a``: any tensor whose storage holds the bf16 planes of the M x K operand from byte ``a_offset`` on (16-byte aligned) -
    e.g. the scratch of the persistent backward recurrence (``ptmi_lstm_handoff_cols``)."""
    _gemm_planes_call('ptmi_gemm_planes_bf16', 'gemm_planes_bf16', out, M, N, K, split_k,
                      (a.data_ptr() + a_offset, b.data_ptr(), _lib.ptr(bias), out.data_ptr(), max(out.stride(0), N), M, N, K, int(accumulate)))


@_register('gemm_planes_bf16_two_(Tensor(a!) out, Tensor(b!) out2, Tensor a, int a_offset, Tensor b, int M, int N, int K, bool accumulate, '
           'int split_k) -> ()')
def gemm_planes_bf16_two_(out, out2, a, a_offset, b, M, N, K, accumulate, split_k):
    """``[out; out2] (+)= A B^T`` (``ptmi_gemm_planes_bf16_two``): ``out`` takes the first ``out.shape[0]`` rows of the M x N product,
    ``out2`` the rest - two parameters' gradient buffers with one row stride (both directions' ``dW_ih`` of a BLSTM layer)."""
    assert out.shape[0] + out2.shape[0] == M and out.shape[1] == out2.shape[1] == N and out.stride(0) == out2.stride(0), (out.shape, out2.shape)
    _gemm_planes_call('ptmi_gemm_planes_bf16_two', 'gemm_planes_bf16', out, M, N, K, split_k,
                      (a.data_ptr() + a_offset, b.data_ptr(), out.data_ptr(), out2.data_ptr(), out.shape[0], max(out.stride(0), N), M, N, K,
                       int(accumulate)))


@_register('pack_planes_bf16_list(Tensor[] xs) -> Tensor[]')
def pack_planes_bf16_list(xs):
    """Every ``x [k, c_i]`` of up to three sources with one ``k`` -> bf16 (hi, lo) planes of the ``c_i x k`` operand, ONE launch
    (``ptmi_pack_planes_t_bf16_list``): bit for bit ``pack_planes_bf16(x, True)`` of each."""
    lib = _lib.load()
    n, k = len(xs), xs[0].shape[0]
    assert 1 <= n <= 3 and all(x.dim() == 2 and x.shape[0] == k and x.dtype == torch.float32 and (x.stride(1) == 1 or x.shape[1] == 1)
                               for x in xs), [tuple(x.shape) for x in xs]
    outs = [torch.empty(int(lib.ptmi_planes_elems(x.shape[1], k)), dtype=torch.bfloat16, device=x.device) for x in xs]
    src = (ctypes.c_void_p * n)(*[x.data_ptr() for x in xs])
    dst = (ctypes.c_void_p * n)(*[o.data_ptr() for o in outs])
    cols = _lib.int64s(*[x.shape[1] for x in xs])
    ld = _lib.int64s(*[_ld(x) for x in xs])
    _lib.call('ptmi_pack_planes_t_bf16_list', src, cols, ld, dst, n, k, _lib.stream(xs[0].device),
              timer=f'pack_planes_bf16_list:{k}x{sum(x.shape[1] for x in xs)}')
    return outs


@_register('gemm_planes_bf16_group_(Tensor(a!)[] outs, int[] blocks, Tensor a, int a_offset, int M, int m_split, Tensor[] bs, int[] ns, '
           'int K, bool accumulate, int split_k) -> bool')
def gemm_planes_bf16_group_(outs, blocks, a, a_offset, M, m_split, bs, ns, K, accumulate, split_k):
    """The products of the blocks ``(part, segment)`` = ``divmod(blocks[i], len(bs))`` of ``A`` (two parts: rows below / from
    ``m_split``) and the B segments ``bs`` (planes of ``ns[s] x K``), ``outs[i] (+)= A_part B_s^T``, in ONE launch and one slab
    reduction (``ptmi_gemm_planes_bf16_group``); blocks not listed are skipped.  ``a`` / ``a_offset`` as in ``gemm_planes_bf16_``.
    ``False`` - nothing launched - where the big-tile path is not possible: the caller issues separate calls."""
    lib = _lib.load()
    S = len(bs)
    assert len(outs) == len(blocks) and len(ns) == S and len(set(blocks)) == len(blocks), (len(outs), blocks, ns)
    c = (ctypes.c_void_p * (2 * S))()
    ldc = (ctypes.c_int64 * (2 * S))()
    for o, blk in zip(outs, blocks):
        p, s = divmod(int(blk), S)
        assert p in (0, 1) and o.dtype == torch.float32 and o.shape == ((M - m_split) if p else m_split, ns[s]) and o.stride(1) == 1, \
            (blk, o.shape, o.stride())
        c[blk] = o.data_ptr()
        ldc[blk] = max(o.stride(0), ns[s])
    n = (ctypes.c_int32 * S)(*[int(v) for v in ns])
    b = (ctypes.c_void_p * S)(*[t.data_ptr() for t in bs])
    if int(lib.ptmi_gemm_planes_group_plan(M, m_split, n, S, c, K, split_k)) // 100 == 5:
        return False
    ws = torch.empty(int(lib.ptmi_gemm_planes_group_workspace_elems(M, m_split, n, S, c, K, split_k)), dtype=torch.float32, device=a.device)
    shape = f'{M}/{m_split}x{"+".join(str(int(v)) for v in ns)}x{K}'
    return 0 == _lib.call('ptmi_gemm_planes_bf16_group', a.data_ptr() + a_offset, M, m_split, b, n, S, c, ldc, K, int(accumulate), split_k,
                          _products(), ws.data_ptr(), _lib.stream(a.device), timer=f'gemm_group_bf16:{shape}:{split_k}', accept=(-2,))


# ------------------------------------------------------------------------------------------------ unit norm
@_register('unit_norm_forward(Tensor x, float eps) -> (Tensor, Tensor)')
def unit_norm_forward(x, eps):
    N, E, F = x.shape
    y = torch.empty_like(x)
    inv = torch.empty((N, F), dtype=torch.float32, device=x.device)
    _lib.call('ptmi_unit_norm_forward', _lib.ptr(x), _lib.ptr(y), _lib.ptr(inv), N, E, F, eps, _lib.stream(x.device),
              timer='unit_norm_forward')
    return y, inv


@_register('unit_norm_backward(Tensor gy, Tensor y, Tensor inv, float eps) -> Tensor')
def unit_norm_backward(gy, y, inv, eps):
    N, E, F = y.shape
    dx = torch.empty_like(y)
    _lib.call('ptmi_unit_norm_backward', _lib.ptr(gy), _lib.ptr(y), _lib.ptr(inv), _lib.ptr(dx), N, E, F, eps, _lib.stream(y.device),
              timer='unit_norm_backward')
    return dx


# ------------------------------------------------------------------------------------------------ (B)LSTM recurrence
@_register('lstm_recurrence_forward(Tensor(a!) gates, Tensor(b!) hy, Tensor? c0, Tensor w_hh_pad, Tensor? w_amax, Tensor bs_dev, '
           'Tensor offs_dev, int bs_host, int offs_host, int T, int max_batch, int rows, int H, int KP, int ndir, bool persistent, '
           'Tensor(c!)? scratch=None, bool prefilled=False, Tensor(d!)? backward_scratch=None, Tensor? step_masks=None) -> (Tensor, Tensor?)')
def lstm_recurrence_forward(gates, hy, c0, w_hh_pad, w_amax, bs_dev, offs_dev, bs_host, offs_host, T, max_batch, rows, H, KP, ndir,
                            persistent, scratch=None, prefilled=False, backward_scratch=None, step_masks=None):
    """gates: pre-activations in, activations out (in place); hy: output rows (a view into the caller's padded buffer).
    Returns (c, scratch): scratch = the persistent kernel's flag / hand-off buffer (its last 8 words are the watchdog
    words), None when the one-launch-per-timestep kernels ran.  bs_host / offs_host: addresses of the HOST copies of the
    batch-size / offset vectors (the per-step launcher takes them as kernel arguments)."""
    lib = _lib.load()
    dev = gates.device
    st = _lib.stream(dev)
    # row-slot batches (step_masks): idle rows are not written - they must read as zeros
    c = (torch.zeros if step_masks is not None else torch.empty)((rows, ndir * H), dtype=torch.float32, device=dev)
    rc = -2
    flags = None
    if persistent:
        n = int(lib.ptmi_lstm_scratch_elems(T, ndir, max_batch, H, 0))
        flags = scratch if scratch is not None else torch.empty(n, dtype=torch.int32, device=dev)
        assert flags.numel() >= n and flags.dtype == torch.int32
        assert step_masks is None or (step_masks.dtype == torch.int64 and step_masks.numel() == 3 * T)
        rc = _lib.call('ptmi_lstm_forward_persistent', gates.data_ptr(), hy.data_ptr(), c.data_ptr(), _lib.ptr(c0), w_hh_pad.data_ptr(),
                       _lib.ptr(w_amax), bs_dev.data_ptr(), offs_dev.data_ptr(), _lib.ptr(step_masks), flags.data_ptr(), T, max_batch, rows,
                       H, KP, ndir, int(bool(prefilled and scratch is not None)), _lib.ptr(backward_scratch), st, timer='lstm_forward',
                       accept=(-2,) if step_masks is None else ())          # (a row-slot batch has no step-per-launch form)
    if rc == -2:        # configuration not resident-able: one launch per timestep
        flags = None
        _lib.call('ptmi_lstm_forward', gates.data_ptr(), hy.data_ptr(), c.data_ptr(), _lib.ptr(c0), w_hh_pad.data_ptr(),
                  ctypes.c_void_p(bs_host), ctypes.c_void_p(offs_host), T, max_batch, H, KP, ndir, st, timer='lstm_forward')
    return c, flags


@_register('lstm_recurrence_backward(Tensor gates, Tensor c, Tensor? c0, Tensor dhy, Tensor w_hh_t, Tensor bs_dev, Tensor offs_dev, '
           'int bs_host, int offs_host, int T, int max_batch, int rows, int H, int ndir, bool persistent, Tensor(a!)? scratch=None, '
           'int prefilled=0, Tensor? step_masks=None) -> (Tensor, Tensor?)')
def lstm_recurrence_backward(gates, c, c0, dhy, w_hh_t, bs_dev, offs_dev, bs_host, offs_host, T, max_batch, rows, H, ndir, persistent,
                             scratch=None, prefilled=0, step_masks=None):
    """Returns (dgates, scratch): scratch as above; behind its tile-major copy it carries the bias gradient [ndir * 4H]
    and, for the split kernels, the word with max |dgates| (see ``ops.lstm``)."""
    lib = _lib.load()
    dev = gates.device
    dg = torch.empty_like(gates)
    flags = None
    if persistent:
        n = int(lib.ptmi_lstm_scratch_elems(T, ndir, max_batch, H, 1))
        flags = scratch if scratch is not None else torch.empty(n, dtype=torch.int32, device=dev)
        assert flags.numel() >= n and flags.dtype == torch.int32
        persistent = _lstm_backward_persistent(gates, c, c0, dhy, w_hh_t, dg, None, flags, None, bs_dev, offs_dev, T, max_batch, rows, H,
                                               ndir, 0, T, int(prefilled) if scratch is not None else 0, step_masks=step_masks)
        if not persistent and step_masks is not None:          # (a row-slot batch has no step-per-launch form)
            _lib.check(-2, 'ptmi_lstm_backward_persistent')
    if not persistent:
        flags = None
        dcs = torch.empty((max_batch, ndir, H), dtype=torch.float32, device=dev)
        _lib.call('ptmi_lstm_backward', gates.data_ptr(), c.data_ptr(), _lib.ptr(c0), dhy.data_ptr(), w_hh_t.data_ptr(), dg.data_ptr(),
                  dcs.data_ptr(), ctypes.c_void_p(bs_host), ctypes.c_void_p(offs_host), T, max_batch, H, ndir, _lib.stream(dev),
                  timer='lstm_backward')
    return dg, flags


# ------------------------------------------------------------------------------------------------ dual-path RNN (csrc/dprnn.hip)
def _i32c(*tensors):
    for t in tensors:
        assert t is None or (t.is_contiguous() and t.dtype == torch.int32 and t.is_cuda), (t.shape, t.stride(), t.dtype, t.device)


@_register('dprnn_tables(Tensor like, Tensor? lengths, int B, int S, int K, int P) -> (Tensor, Tensor, Tensor)')
def dprnn_tables(like, lengths, B, S, K, P):
    """``(chunks [B], intra [B S, 3], inter [B K, 3])`` (int32) on ``like``'s device: the chunk counts ``S_b`` of ``lengths`` (frames,
    device memory; None: ``S``) and the sequence tables of both paths (``ptmi_dprnn_tables``)."""
    lengths, is64 = _lengths(lengths, B)
    dev = like.device
    chunks = torch.empty(B, dtype=torch.int32, device=dev)
    intra = torch.empty((B * S, 3), dtype=torch.int32, device=dev)
    inter = torch.empty((B * K, 3), dtype=torch.int32, device=dev)
    _lib.call('ptmi_dprnn_tables', _lib.ptr(lengths), is64, B, S, K, P, chunks.data_ptr(), intra.data_ptr(), inter.data_ptr(),
              _lib.stream(dev), timer='dprnn_tables')
    return chunks, intra, inter


def _chunk_lstm_dims(gates, table, H):
    _f32c(gates)
    _i32c(table)
    assert gates.dim() == 2 and table.dim() == 2 and table.shape[1] == 3 and gates.shape[1] % (4 * H) == 0, (gates.shape, table.shape, H)
    ndir = gates.shape[1] // (4 * H)
    assert ndir in (1, 2), gates.shape
    return gates.shape[0], ndir


@_register('chunk_lstm_forward(Tensor(a!) gates, Tensor w_hh, Tensor? w_hh_reverse, Tensor b_hh, Tensor? b_hh_reverse, Tensor table, '
           'int cap, int H) -> (Tensor, Tensor)')
def chunk_lstm_forward(gates, w_hh, w_hh_reverse, b_hh, b_hh_reverse, table, cap, H):
    """The time loop of one LSTM layer over the sequences of ``table [nseq, 3]`` = (base row, step stride, step count): ``gates [rows,
    ndir 4H]`` holds ``x W_ih^T + b_ih`` and becomes the activated gates; returns ``(h, c) [rows, ndir H]`` (``ptmi_chunk_lstm_forward``).
    Every row ``base + t stride``, ``t < cap``, must lie inside ``rows``: the caller's tables guarantee it."""
    rows, ndir = _chunk_lstm_dims(gates, table, H)
    _f32c(w_hh, w_hh_reverse, b_hh, b_hh_reverse)
    assert w_hh.shape == (4 * H, H) and b_hh.shape == (4 * H,) and (ndir == 1 or (w_hh_reverse.shape == (4 * H, H)
                                                                                  and b_hh_reverse.shape == (4 * H,)))
    h = torch.empty((rows, ndir * H), dtype=torch.float32, device=gates.device)
    c = torch.empty((rows, ndir * H), dtype=torch.float32, device=gates.device)
    _lib.call('ptmi_chunk_lstm_forward', gates.data_ptr(), w_hh.data_ptr(), _lib.ptr(w_hh_reverse), b_hh.data_ptr(), _lib.ptr(b_hh_reverse),
              h.data_ptr(), c.data_ptr(), table.data_ptr(), table.shape[0], cap, H, ndir, _lib.stream(gates.device),
              timer=f'chunk_lstm_forward:{table.shape[0]}x{cap}x{H}')
    return h, c


@_register('chunk_lstm_backward(Tensor(a!) gates, Tensor dh, Tensor w_hh, Tensor? w_hh_reverse, Tensor h, Tensor c, Tensor table, '
           'int cap, int H) -> Tensor')
def chunk_lstm_backward(gates, dh, w_hh, w_hh_reverse, h, c, table, cap, H):
    """``gates`` (the forward's activated gates) becomes ``d gates``; returns ``hprev [rows, ndir H]``, the ``h`` of every row's step
    before (``ptmi_chunk_lstm_backward``)."""
    rows, ndir = _chunk_lstm_dims(gates, table, H)
    _f32c(dh, w_hh, w_hh_reverse, h, c)
    assert dh.shape == h.shape == c.shape == (rows, ndir * H), (dh.shape, h.shape, c.shape)
    hprev = torch.empty_like(h)
    _lib.call('ptmi_chunk_lstm_backward', gates.data_ptr(), dh.data_ptr(), w_hh.data_ptr(), _lib.ptr(w_hh_reverse), h.data_ptr(),
              c.data_ptr(), hprev.data_ptr(), table.data_ptr(), table.shape[0], cap, H, ndir, _lib.stream(gates.device),
              timer=f'chunk_lstm_backward:{table.shape[0]}x{cap}x{H}')
    return hprev


def _dprnn_colsum(x, twice):
    lib = _lib.load()
    assert x.dim() == 2 and x.dtype == torch.float32 and (x.stride(1) == 1 or x.shape[1] == 1), (x.shape, x.stride(), x.dtype)
    rows, C = x.shape
    out = torch.empty(C, dtype=torch.float32, device=x.device)
    out2 = torch.empty(C, dtype=torch.float32, device=x.device) if twice else None
    ws = _doubles(lib.ptmi_dprnn_colsum_workspace_elems(rows, C), x.device)
    _lib.call('ptmi_dprnn_colsum', x.data_ptr(), _ld(x), out.data_ptr(), _lib.ptr(out2), ws.data_ptr(), rows, C, _lib.stream(x.device),
              timer='dprnn_colsum')
    return out, out2


@_register('dprnn_colsum(Tensor x) -> Tensor')
def dprnn_colsum(x):
    """``x [rows, C]`` (unit inner stride, any row stride) -> ``[C]``: the column sums, fp64 inside, in a fixed order (``ptmi_dprnn_colsum``)."""
    return _dprnn_colsum(x, False)[0]


@_register('dprnn_colsum_pair(Tensor x) -> (Tensor, Tensor)')
def dprnn_colsum_pair(x):
    """:func:`dprnn_colsum` into two tensors of the same content - the gradients of ``b_ih`` and ``b_hh`` - with one pass over the rows."""
    return _dprnn_colsum(x, True)


@_register('dprnn_norm_residual_forward(Tensor z, Tensor residual, Tensor gamma, Tensor beta, Tensor? chunks, int S, int K, float eps) '
           '-> (Tensor, Tensor)')
def dprnn_norm_residual_forward(z, residual, gamma, beta, chunks, S, K, eps):
    """``z [B S K, N]`` -> ``(y, stats [rows, 2])``: the layer norm over ``N`` on the rows ``(b, s, k)`` with ``s < chunks[b]``, zeros on
    the others, plus ``residual`` (``ptmi_dprnn_norm_residual_forward``)."""
    _f32c(z, residual, gamma, beta)
    _i32c(chunks)
    rows, N = z.shape
    assert residual.shape == z.shape and gamma.numel() == N and beta.numel() == N and rows % (S * K) == 0
    assert chunks is None or chunks.numel() == rows // (S * K)
    y = torch.empty_like(z)
    stats = torch.empty((rows, 2), dtype=torch.float32, device=z.device)
    _lib.call('ptmi_dprnn_norm_residual_forward', z.data_ptr(), residual.data_ptr(), gamma.data_ptr(), beta.data_ptr(), _lib.ptr(chunks),
              y.data_ptr(), stats.data_ptr(), rows, N, S, K, eps, _lib.stream(z.device), timer='dprnn_norm_residual_forward')
    return y, stats


@_register('dprnn_norm_residual_backward(Tensor gy, Tensor z, Tensor stats, Tensor gamma, Tensor? chunks, int S, int K) '
           '-> (Tensor, Tensor, Tensor)')
def dprnn_norm_residual_backward(gy, z, stats, gamma, chunks, S, K):
    """``(dz, dresidual, dparams [2 N])``: ``d gamma | d beta`` over the valid rows (``ptmi_dprnn_norm_residual_backward``)."""
    lib = _lib.load()
    _f32c(gy, z, stats, gamma)
    _i32c(chunks)
    rows, N = z.shape
    assert gy.shape == z.shape and stats.shape == (rows, 2) and gamma.numel() == N and rows % (S * K) == 0
    dz, dres = torch.empty_like(z), torch.empty_like(z)
    dparams = torch.empty(2 * N, dtype=torch.float32, device=z.device)
    ws = _doubles(lib.ptmi_dprnn_colsum_workspace_elems(rows, N), z.device)
    _lib.call('ptmi_dprnn_norm_residual_backward', gy.data_ptr(), z.data_ptr(), stats.data_ptr(), gamma.data_ptr(), _lib.ptr(chunks),
              dz.data_ptr(), dres.data_ptr(), dparams.data_ptr(), ws.data_ptr(), rows, N, S, K, _lib.stream(z.device),
              timer='dprnn_norm_residual_backward')
    return dz, dres, dparams


@_register('dprnn_segment(Tensor x, int K, int P) -> Tensor')
def dprnn_segment(x, K, P):
    """``x [B, L, N]`` (any strides) -> ``[B, S, K, N]``: windows of ``K`` frames every ``P`` of the signal with ``K - P`` zero frames in
    front and behind, the last window padded (``ptmi_dprnn_segment``)."""
    lib = _lib.load()
    assert x.dim() == 3 and x.dtype == torch.float32 and 1 <= P <= K, (x.shape, x.dtype, K, P)
    B, L, N = x.shape
    S = int(lib.ptmi_dprnn_num_chunks(L, K, P))
    seg = torch.empty((B, S, K, N), dtype=torch.float32, device=x.device)
    strides = _lib.int64s(*x.stride())
    _lib.call('ptmi_dprnn_segment', x.data_ptr(), strides, seg.data_ptr(), B, L, N, S, K, P, _lib.stream(x.device), timer='dprnn_segment')
    return seg


@_register('dprnn_overlap_add(Tensor seg, int P, int L_out, int front) -> Tensor')
def dprnn_overlap_add(seg, P, L_out, front):
    """``seg [B, S, K, N]`` (any strides) -> ``[B, L_out, N]``: frame ``l`` is the sum of the window elements that hold frame ``l +
    front`` of the padded signal; ``front = K - P``: those :func:`dprnn_segment` copies frame ``l`` to (``ptmi_dprnn_overlap_add``);
    ``L_out + front <= (S - 1) P + K``."""
    assert seg.dim() == 4 and seg.dtype == torch.float32, (seg.shape, seg.dtype)
    B, S, K, N = seg.shape
    out = torch.empty((B, L_out, N), dtype=torch.float32, device=seg.device)
    strides = _lib.int64s(*seg.stride())
    _lib.call('ptmi_dprnn_overlap_add', seg.data_ptr(), strides, out.data_ptr(), B, L_out, N, S, K, P, front, _lib.stream(seg.device),
              timer='dprnn_overlap_add')
    return out


# ------------------------------------------------------------------------------------------------ Griffin-Lim (csrc/griffin_lim.hip)
#: the sizes the register-FFT plans of csrc/stft.hip cover: ``ptmi_gl_stft_update`` (the fused update) exists for these
GL_PLAN_SIZES = (64, 128, 256, 512, 1024, 2048)


def _gl_check(a, *specs):
    assert a.dtype == torch.float32 and a.is_contiguous(), (a.dtype, a.is_contiguous())
    for s in specs:
        assert s.dtype == torch.float32 and s.is_contiguous() and tuple(s.shape) == (*a.shape, 2), (s.dtype, s.shape, a.shape)


@_register('gl_project(Tensor a, Tensor y) -> Tensor')
def gl_project(a, y):
    """``P = a y / |y|`` (``angle(0) := 0``): ``a [...]`` fp32, ``y [..., 2]`` interleaved fp32 -> ``P [..., 2]`` (``ptmi_gl_project``;
    griffin_lim.py:55-56, 151-152)."""
    _gl_check(a, y)
    P = torch.empty_like(y)
    _lib.call('ptmi_gl_project', a.data_ptr(), y.data_ptr(), a.numel(), P.data_ptr(), _lib.stream(a.device), timer='gl_project')
    return P


@_register('gl_project_backward(Tensor g, Tensor y) -> Tensor')
def gl_project_backward(g, y):
    """``d a = Re(conj(y / |y|) g)``: the adjoint of :func:`gl_project` in ``a`` (``ptmi_gl_project_backward``)."""
    assert g.dtype == y.dtype == torch.float32 and g.is_contiguous() and y.is_contiguous() and g.shape == y.shape and g.shape[-1] == 2
    da = torch.empty(g.shape[:-1], dtype=torch.float32, device=g.device)
    _lib.call('ptmi_gl_project_backward', g.data_ptr(), y.data_ptr(), da.numel(), da.data_ptr(), _lib.stream(g.device),
              timer='gl_project_backward')
    return da


def gl_state(device, iterations):
    """The device state of one retrieval: ``(state int32 [4] = done, num_iterations, nparts, reserved; partials fp64; rmse fp32
    [iterations], NaN)``."""
    state = torch.zeros(4, dtype=torch.int32, device=device)
    partials = torch.zeros(int(_lib.load().ptmi_gl_partials_elems()), dtype=torch.float64, device=device)
    rmse = torch.full((iterations,), float('nan'), dtype=torch.float32, device=device)
    return state, partials, rmse


@_register('gl_update(Tensor xnew, Tensor(a!) x, Tensor a, float alpha, Tensor(b!) P, Tensor(c!) partials, Tensor(d!) state) -> ()')
def gl_update(xnew, x, a, alpha, P, partials, state):
    """griffin_lim.py:137-142, unfused: ``y = xnew + alpha (xnew - x)``; ``x <- xnew`` in place; ``P <- a y / |y|``; the workgroups' fp64
    partial sums of ``(|xnew| - a)^2`` into ``partials`` and their count into ``state[2]``.  Nothing is written once ``state[0]`` (done)
    is set (``ptmi_gl_update``)."""
    _gl_check(a, xnew, x, P)
    assert partials.dtype == torch.float64 and partials.numel() >= _lib.load().ptmi_gl_partials_elems() and state.dtype == torch.int32
    _lib.call('ptmi_gl_update', xnew.data_ptr(), x.data_ptr(), a.data_ptr(), a.numel(), alpha, P.data_ptr(), partials.data_ptr(),
              state.data_ptr(), _lib.stream(a.device), timer='gl_update')


@_register('gl_iterations(Tensor a, Tensor(a!) x, Tensor(b!) P, Tensor syn, Tensor window, Tensor twiddle, int[] geom, int samples, '
           'float alpha, int iterations, float atol, bool fused, int poll, Tensor(c!) rmse, Tensor(d!) partials, Tensor(e!) state) -> ()')
def gl_iterations(a, x, P, syn, window, twiddle, geom, samples, alpha, iterations, atol, fused, poll, rmse, partials, state):
    """The loop of griffin_lim.py:135-150 on device state: per iteration ``audio = iSTFT(P)`` (``ptmi_istft_forward``), the update
    (``fused``: ``ptmi_gl_stft_update``, one launch; otherwise ``ptmi_stft_forward`` + ``ptmi_gl_update``) and ``ptmi_gl_finish``
    (``rmse[n]``, ``state[0]`` = done, ``state[1]`` = iterations run).  ``a [rows, frames, F]``; ``x``, ``P [rows, frames, F, 2]`` hold
    the start on entry (``P = a y / |y|`` of the start ``y``) and the last live iteration's values on return.  No host read inside the
    loop unless ``poll > 0``: then ``state[0]`` is read every ``poll`` iterations and the launches stop once it is set (they would
    write nothing).  The audio and (unfused) spectrum buffers are allocated once, in front of the loop."""
    lib = _lib.load()
    _gl_check(a, x, P)
    rows, frames, F = a.shape
    assert F == geom[0] // 2 + 1 and rmse.numel() >= iterations and state.dtype == torch.int32
    assert partials.dtype == torch.float64 and partials.numel() >= lib.ptmi_gl_partials_elems()
    g = _geom(geom)
    assert lib.ptmi_stft_num_frames(g, samples) == frames, (samples, frames)
    if iterations <= 0:
        return
    dev, st = a.device, _lib.stream(a.device)
    audio = torch.empty((rows, samples), dtype=torch.float32, device=dev)
    xnew = None if fused else torch.empty_like(x)
    n = a.numel()
    for it in range(iterations):
        _lib.call('ptmi_istft_forward', P.data_ptr(), rows, frames, None, syn.data_ptr(), twiddle.data_ptr(), g, 0, 1.0, geom[3], samples,
                  samples, audio.data_ptr(), st, timer='gl_istft')
        if fused:
            _lib.call('ptmi_gl_stft_update', audio.data_ptr(), rows, samples, samples, window.data_ptr(), twiddle.data_ptr(), g, frames,
                      alpha, x.data_ptr(), a.data_ptr(), P.data_ptr(), partials.data_ptr(), state.data_ptr(), st, timer='gl_stft_update')
        else:
            _lib.call('ptmi_stft_forward', audio.data_ptr(), rows, samples, samples, None, window.data_ptr(), twiddle.data_ptr(), g, frames,
                      0, 1.0, xnew.data_ptr(), st, timer='gl_stft')
            _lib.call('ptmi_gl_update', xnew.data_ptr(), x.data_ptr(), a.data_ptr(), n, alpha, P.data_ptr(), partials.data_ptr(),
                      state.data_ptr(), st, timer='gl_update')
        _lib.call('ptmi_gl_finish', partials.data_ptr(), n, atol, it, rmse.data_ptr(), state.data_ptr(), st, timer='gl_finish')
        if poll > 0 and (it + 1) % poll == 0 and it + 1 < iterations and int(state[0].item()) != 0:
            break


# ------------------------------------------------------------------------------------------------ anti-aliased activation (BigVGAN)
def _aa_args(x, up_filter, down_filter, alpha, beta):
    assert x.dim() == 3 and x.dtype == torch.float32 and x.is_contiguous(), (x.shape, x.dtype, x.is_contiguous())
    C = x.shape[1]
    for f in (up_filter, down_filter):
        assert f is None or (f.dim() == 1 and f.dtype == torch.float32 and f.is_contiguous() and f.device == x.device), f
    assert (alpha is None) == (beta is None)
    for p in (alpha, beta):
        assert p is None or (tuple(p.shape) == (C,) and p.dtype == torch.float32 and p.is_contiguous() and p.device == x.device), p
    return x.shape[0], C, x.shape[2], 0 if up_filter is None else up_filter.numel(), 0 if down_filter is None else down_filter.numel()


@_register('anti_alias_forward(Tensor x, Tensor? up_filter, Tensor? down_filter, Tensor? alpha, Tensor? beta, int up_ratio, '
           'int down_ratio, bool padding, bool logscale) -> Tensor')
def anti_alias_forward(x, up_filter, down_filter, alpha, beta, up_ratio, down_ratio, padding, logscale):
    """``x [B, C, T]`` -> ``[B, C, M]``: up-sampling by ``up_filter`` (None: off), Snake with ``alpha`` / ``beta [C]`` (None: off), low-pass
    and decimation by ``down_filter`` (None: off), one launch (``ptmi_anti_alias_forward``; alias_free_activation/torch/act.py:25-30)."""
    B, C, T, k, dk = _aa_args(x, up_filter, down_filter, alpha, beta)
    lib = _lib.load()
    M = lib.ptmi_anti_alias_out_len(T, up_ratio, k, down_ratio, dk, int(padding))
    assert M >= 0, (T, up_ratio, k, down_ratio, dk, padding)
    y = torch.empty((B, C, M), dtype=torch.float32, device=x.device)
    if y.numel():
        _lib.call('ptmi_anti_alias_forward', x.data_ptr(), _lib.ptr(up_filter), _lib.ptr(down_filter), _lib.ptr(alpha), _lib.ptr(beta), B,
                  C, T, up_ratio, k, down_ratio, dk, int(padding), int(alpha is not None), int(logscale), y.data_ptr(),
                  _lib.stream(x.device), timer='anti_alias_forward')
    return y


@_register('anti_alias_backward(Tensor dy, Tensor x, Tensor? up_filter, Tensor? down_filter, Tensor? alpha, Tensor? beta, int up_ratio, '
           'int down_ratio, bool padding, bool logscale, int param_grads) -> (Tensor, Tensor, Tensor)')
def anti_alias_backward(dy, x, up_filter, down_filter, alpha, beta, up_ratio, down_ratio, padding, logscale, param_grads):
    """The adjoint of :func:`anti_alias_forward`: ``(dx, dalpha, dbeta)``.  ``param_grads`` 0: none (both empty), 1: one shared parameter
    (Snake: both sums in ``dalpha``, ``dbeta`` empty), 2: ``alpha`` and ``beta`` (``ptmi_anti_alias_backward``)."""
    B, C, T, k, dk = _aa_args(x, up_filter, down_filter, alpha, beta)
    lib = _lib.load()
    M = lib.ptmi_anti_alias_out_len(T, up_ratio, k, down_ratio, dk, int(padding))
    assert dy.dtype == torch.float32 and dy.is_contiguous() and tuple(dy.shape) == (B, C, M), (dy.shape, dy.dtype, (B, C, M))
    assert param_grads in (0, 1, 2) and (param_grads == 0 or alpha is not None)
    dx = torch.empty_like(x)
    dalpha = torch.empty(C if param_grads >= 1 else 0, dtype=torch.float32, device=x.device)
    dbeta = torch.empty(C if param_grads == 2 else 0, dtype=torch.float32, device=x.device)
    if M == 0 or dx.numel() == 0:
        return dx.zero_(), dalpha.zero_(), dbeta.zero_()
    ws = None
    if param_grads:
        ws = torch.empty(lib.ptmi_anti_alias_workspace_elems(B, C, T, up_ratio, k, down_ratio, dk, int(padding)), dtype=torch.float64,
                         device=x.device)
    _lib.call('ptmi_anti_alias_backward', dy.data_ptr(), x.data_ptr(), _lib.ptr(up_filter), _lib.ptr(down_filter), _lib.ptr(alpha),
              _lib.ptr(beta), B, C, T, up_ratio, k, down_ratio, dk, int(padding), int(alpha is not None), int(logscale), dx.data_ptr(),
              dalpha.data_ptr() if param_grads >= 1 else None, dbeta.data_ptr() if param_grads == 2 else None, _lib.ptr(ws),
              _lib.stream(x.device), timer='anti_alias_backward')
    return dx, dalpha, dbeta


# ------------------------------------------------------------------------------------------------ WaveNet vocoder
def _f32c(*tensors):
    for t in tensors:
        assert t is None or (t.dtype == torch.float32 and t.is_contiguous()), (t.shape, t.dtype, t.stride())


@_register('mu_law_encode(Tensor x, int mu_quantization) -> Tensor')
def mu_law_encode(x, mu_quantization):
    """``x`` (fp32, any shape) -> int64 codes in ``[0, mu_quantization - 1]`` (``ptmi_mu_law_encode``; ops/mu_law.py:22-29)."""
    _f32c(x)
    codes = torch.empty(x.shape, dtype=torch.int64, device=x.device)
    if x.numel():
        _lib.call('ptmi_mu_law_encode', x.data_ptr(), x.numel(), mu_quantization, codes.data_ptr(), _lib.stream(x.device), timer='mu_law_encode')
    return codes


@_register('mu_law_decode(Tensor codes, int mu_quantization) -> Tensor')
def mu_law_decode(codes, mu_quantization):
    """int64 or fp32 codes -> fp32 signal in ``[-1, 1]`` (``ptmi_mu_law_decode``; ops/mu_law.py:10-19)."""
    assert codes.dtype in (torch.int64, torch.float32) and codes.is_contiguous(), (codes.dtype, codes.stride())
    out = torch.empty(codes.shape, dtype=torch.float32, device=codes.device)
    if codes.numel():
        _lib.call('ptmi_mu_law_decode', codes.data_ptr(), int(codes.dtype == torch.float32), codes.numel(), mu_quantization, out.data_ptr(),
                  _lib.stream(codes.device), timer='mu_law_decode')
    return out


@_register('wavenet_embed_forward(Tensor audio, Tensor embed) -> (Tensor, Tensor)')
def wavenet_embed_forward(audio, embed):
    """``audio [B, T]``, ``embed [A, R]`` -> ``(codes [B, T] int64, x0 [B, T, R])``, one launch (``ptmi_wavenet_embed_forward``)."""
    _f32c(audio, embed)
    assert audio.dim() == 2 and embed.dim() == 2 and audio.numel() > 0
    A, R = embed.shape
    codes = torch.empty(audio.shape, dtype=torch.int64, device=audio.device)
    x0 = torch.empty((*audio.shape, R), dtype=torch.float32, device=audio.device)
    _lib.call('ptmi_wavenet_embed_forward', audio.data_ptr(), embed.data_ptr(), audio.numel(), A, R, codes.data_ptr(), x0.data_ptr(),
              _lib.stream(audio.device), timer='wavenet_embed_forward')
    return codes, x0


@_register('wavenet_embed_backward(Tensor dx0, Tensor codes, int A) -> Tensor')
def wavenet_embed_backward(dx0, codes, A):
    """``dembed [A, R]``: the rows of ``dx0 [B, T, R]`` summed per code in one fixed order (``ptmi_wavenet_embed_backward``)."""
    _f32c(dx0)
    assert codes.dtype == torch.int64 and codes.is_contiguous() and dx0.shape[:-1] == codes.shape
    n, R = codes.numel(), dx0.shape[-1]
    lib = _lib.load()
    ws = torch.empty(lib.ptmi_wavenet_embed_workspace_elems(n, A, R), dtype=torch.float64, device=dx0.device)
    out = torch.empty((A, R), dtype=torch.float32, device=dx0.device)
    _lib.call('ptmi_wavenet_embed_backward', dx0.data_ptr(), codes.data_ptr(), n, A, R, out.data_ptr(), ws.data_ptr(), _lib.stream(dx0.device),
              timer='wavenet_embed_backward')
    return out


@_register('wavenet_colsum(Tensor x) -> Tensor')
def wavenet_colsum(x):
    """``x [rows, width]`` (unit inner stride, any row stride) -> ``[width]``: column sums in fp64, one fixed order (``ptmi_wavenet_colsum``)."""
    assert x.dim() == 2 and x.dtype == torch.float32 and (x.stride(1) == 1 or x.shape[1] == 1) and x.numel() > 0, (x.shape, x.stride())
    rows, width = x.shape
    lib = _lib.load()
    ws = torch.empty(lib.ptmi_wavenet_colsum_workspace_elems(rows, width), dtype=torch.float64, device=x.device)
    out = torch.empty(width, dtype=torch.float32, device=x.device)
    _lib.call('ptmi_wavenet_colsum', x.data_ptr(), rows, width, max(x.stride(0), width), out.data_ptr(), ws.data_ptr(), _lib.stream(x.device),
              timer='wavenet_colsum')
    return out


@_register('wavenet_ola_forward(Tensor G, Tensor bias, int B, int Tf, int window, int stride, int front, int Tout) -> Tensor')
def wavenet_ola_forward(G, bias, B, Tf, window, stride, front, Tout):
    """``G [B Tf, C window]`` -> ``[B, Tout, C]``: overlap-add, bias and crop (``ptmi_wavenet_ola_forward``; wavenet.py:186-195)."""
    _f32c(G, bias)
    C = bias.numel()
    assert tuple(G.shape) == (B * Tf, C * window), (G.shape, B, Tf, C, window)
    out = torch.empty((B, Tout, C), dtype=torch.float32, device=G.device)
    _lib.call('ptmi_wavenet_ola_forward', G.data_ptr(), bias.data_ptr(), B, C, Tf, window, stride, front, Tout, out.data_ptr(),
              _lib.stream(G.device), timer='wavenet_ola_forward')
    return out


@_register('wavenet_ola_backward(Tensor dout, int Tf, int window, int stride, int front) -> Tensor')
def wavenet_ola_backward(dout, Tf, window, stride, front):
    """The adjoint of :func:`wavenet_ola_forward` in ``G``: the framing gather ``dG [B Tf, C window]`` (``ptmi_wavenet_ola_backward``)."""
    _f32c(dout)
    B, Tout, C = dout.shape
    dG = torch.empty((B * Tf, C * window), dtype=torch.float32, device=dout.device)
    _lib.call('ptmi_wavenet_ola_backward', dout.data_ptr(), B, C, Tf, window, stride, front, Tout, dG.data_ptr(), _lib.stream(dout.device),
              timer='wavenet_ola_backward')
    return dG


def _rows3(t, width, what):
    """``t [B, T, >= width]`` as (pointer, row stride): unit inner stride, rows ``b T + t`` evenly spaced."""
    assert t.dim() == 3 and t.dtype == torch.float32 and t.shape[2] == width and (t.stride(2) == 1 or width == 1), (what, t.shape, t.stride())
    assert t.shape[0] == 1 or t.stride(0) == t.shape[1] * t.stride(1), (what, t.shape, t.stride())
    return t.data_ptr(), t.stride(1)


@_register('wavenet_gate_forward_(Tensor(a!) acts, Tensor P, Tensor bias, Tensor cond, int dilation) -> ()')
def wavenet_gate_forward_(acts, P, bias, cond, dilation):
    """``acts [B, T, R]`` (a slice of ``acts_all`` or a tensor of its own) ``= tanh(z[:R]) sigmoid(z[R:])``, ``z`` from ``P [B, T, 4R]``,
    ``bias [2R]`` and ``cond [B, T, 2R]`` (a slice of the conditioning GEMM's output) (``ptmi_wavenet_gate_forward``; wavenet.py:152-156)."""
    _f32c(P, bias)
    B, T, R = acts.shape
    assert tuple(P.shape) == (B, T, 4 * R) and bias.numel() == 2 * R, (P.shape, bias.shape, acts.shape)
    ap, lda = _rows3(acts, R, 'acts')
    cp, ldc = _rows3(cond, 2 * R, 'cond')
    assert cond.shape[:2] == acts.shape[:2]
    _lib.call('ptmi_wavenet_gate_forward', P.data_ptr(), bias.data_ptr(), cp, ldc, B, T, R, dilation, ap, lda, _lib.stream(P.device),
              timer='wavenet_gate_forward')


@_register('wavenet_gate_backward_(Tensor(a!) dz, Tensor dacts, Tensor P, Tensor bias, Tensor cond, int dilation, bool want_dP, '
           'bool want_dbias) -> (Tensor, Tensor)')
def wavenet_gate_backward_(dz, dacts, P, bias, cond, dilation, want_dP, want_dbias):
    """``dz [B, T, 2R]`` (a slice of ``dcond``) is written; returns ``(dP [B, T, 4R], dbias [2R])`` (empty when not wanted)
    (``ptmi_wavenet_gate_backward``)."""
    _f32c(P, bias)
    B, T, R = dacts.shape
    assert tuple(P.shape) == (B, T, 4 * R) and bias.numel() == 2 * R
    gp, lda = _rows3(dacts, R, 'dacts')
    cp, ldc = _rows3(cond, 2 * R, 'cond')
    zp, ldd = _rows3(dz, 2 * R, 'dz')
    dev = P.device
    dP = torch.empty((B, T, 4 * R) if want_dP else (0,), dtype=torch.float32, device=dev)
    dbias = torch.empty(2 * R if want_dbias else 0, dtype=torch.float32, device=dev)
    ws = None
    if want_dbias:
        ws = torch.empty(_lib.load().ptmi_wavenet_colsum_workspace_elems(B * T, 2 * R), dtype=torch.float64, device=dev)
    _lib.call('ptmi_wavenet_gate_backward', gp, lda, P.data_ptr(), bias.data_ptr(), cp, ldc, B, T, R, dilation, zp, ldd,
              dP.data_ptr() if want_dP else None, dbias.data_ptr() if want_dbias else None, _lib.ptr(ws), _lib.stream(dev),
              timer='wavenet_gate_backward')
    return dP, dbias


@_register('wavenet_generate_(Tensor(a!) y, Tensor(b!)? logits, Tensor(c!) ring, Tensor(d!) last_code, Tensor packed, Tensor embed, '
           'Tensor cond, Tensor u, Tensor layer_meta, Tensor seq_meta, int S, int A, int ring_rows, int t0, int nsteps) -> ()')
def wavenet_generate_(y, logits, ring, last_code, packed, embed, cond, u, layer_meta, seq_meta, S, A, ring_rows, t0, nsteps):
    """``nsteps`` time steps of the sampling loop from ``t0`` in ONE launch (``ptmi_wavenet_generate``; include/ptmi.h has the layouts)."""
    _f32c(packed, embed, cond, u, ring, logits)
    nseq, Tmax = y.shape
    R, L = embed.shape[1], layer_meta.shape[0]
    ex = _lib.load().ptmi_wavenet_generate_ex()
    groups = -(-nseq // ex)
    assert y.dtype == torch.int64 and y.is_contiguous() and layer_meta.dtype == seq_meta.dtype == last_code.dtype == torch.int32
    assert cond.dim() == 3 and cond.shape[2] == 2 * R * L and u.shape == cond.shape[:2], (cond.shape, u.shape)
    assert tuple(seq_meta.shape) == (nseq, 3) and tuple(layer_meta.shape) == (L, 2) and seq_meta.is_contiguous() and layer_meta.is_contiguous()
    assert ring.numel() == groups * ring_rows * ex * R and last_code.numel() == groups * ex and embed.shape[0] >= A
    assert packed.numel() == L * (4 * R * R + 2 * R + R * (S + R) + S + R) + S * A + A * A, packed.shape
    assert logits is None or tuple(logits.shape) == (nseq, Tmax, A)
    _lib.call('ptmi_wavenet_generate', packed.data_ptr(), embed.data_ptr(), cond.data_ptr(), u.data_ptr(), layer_meta.data_ptr(),
              seq_meta.data_ptr(), nseq, cond.shape[1], L, R, S, A, ring_rows, t0, nsteps, Tmax, ring.data_ptr(), last_code.data_ptr(),
              y.data_ptr(), _lib.ptr(logits), _lib.stream(y.device), timer='wavenet_generate')


# ------------------------------------------------------------------------------------------------ BigVGAN generator (inference)
def _bv_epilogue(out, bias, residual):
    _f32c(out, bias, residual)
    assert out.dim() == 3 and (bias is None or tuple(bias.shape) == (out.shape[1],)), (out.shape, None if bias is None else bias.shape)
    assert residual is None or residual.shape == out.shape, (residual.shape, out.shape)


@_register('bigvgan_taps_(Tensor(a!) out, Tensor P, Tensor? bias, Tensor? residual, int K, int dilation, float scale, bool accumulate) -> ()')
def bigvgan_taps_(out, P, bias, residual, K, dilation, scale, accumulate):
    """``out [B, C_out, T] (+)= scale (sum_k P[:, k C_out + co, t + (k - (K-1)/2) d] + bias + residual)`` behind the GEMM that made
    ``P [B, K C_out, T]`` (``ptmi_bigvgan_taps``; the dilated Conv1d of bigvgan.py:56-88,175-189, conv_pre :286-288)."""
    _f32c(P)
    _bv_epilogue(out, bias, residual)
    B, C_out, T = out.shape
    assert tuple(P.shape) == (B, K * C_out, T), (P.shape, out.shape, K)
    _lib.call('ptmi_bigvgan_taps', P.data_ptr(), _lib.ptr(bias), _lib.ptr(residual), B, C_out, T, K, dilation, scale, int(accumulate),
              out.data_ptr(), _lib.stream(out.device), timer='bigvgan_taps')


@_register('bigvgan_conv_direct_(Tensor(a!) out, Tensor x, Tensor weight, Tensor? bias, Tensor? residual, int dilation, float scale, '
           'bool accumulate) -> ()')
def bigvgan_conv_direct_(out, x, weight, bias, residual, dilation, scale, accumulate):
    """The same convolution and epilogue from ``x [B, C_in, T]`` and ``weight [C_out, C_in, K]`` in fp32 FMAs, no ``P``
    (``ptmi_bigvgan_conv_direct``: narrow layers)."""
    _f32c(x, weight)
    _bv_epilogue(out, bias, residual)
    B, C_out, T = out.shape
    C_in, K = weight.shape[1:]
    assert tuple(x.shape) == (B, C_in, T) and weight.shape[0] == C_out, (x.shape, weight.shape, out.shape)
    _lib.call('ptmi_bigvgan_conv_direct', x.data_ptr(), weight.data_ptr(), _lib.ptr(bias), _lib.ptr(residual), B, C_in, C_out, T, K, dilation,
              scale, int(accumulate), out.data_ptr(), _lib.stream(out.device), timer='bigvgan_conv_direct')


@_register('bigvgan_ola(Tensor G, Tensor? bias, int kernel_size, int stride) -> Tensor')
def bigvgan_ola(G, bias, kernel_size, stride):
    """``G [B, C_out k, T]`` -> ``[B, C_out, (T - 1) u - 2 ((k - u) // 2) + k]``: the overlap-add, bias and crop of the up-sampling
    ConvTranspose1d (``ptmi_bigvgan_ola``; bigvgan.py:302-317)."""
    _f32c(G, bias)
    B, rows, T = G.shape
    C_out = rows // kernel_size
    assert rows == C_out * kernel_size and (bias is None or tuple(bias.shape) == (C_out,)), (G.shape, kernel_size)
    Tout = int(_lib.load().ptmi_bigvgan_ola_out_len(T, kernel_size, stride)) if T else 0
    assert Tout >= 0, (T, kernel_size, stride)
    out = torch.empty((B, C_out, Tout), dtype=torch.float32, device=G.device)
    if out.numel():
        _lib.call('ptmi_bigvgan_ola', G.data_ptr(), _lib.ptr(bias), B, C_out, T, kernel_size, stride, out.data_ptr(), _lib.stream(G.device),
                  timer='bigvgan_ola')
    return out


@_register('bigvgan_post(Tensor x, Tensor weight, Tensor? bias, bool tanh) -> Tensor')
def bigvgan_post(x, weight, bias, tanh):
    """``x [B, C, T]``, ``weight [1, C, K]`` -> ``[B, 1, T]``: conv_post and ``tanh`` / the clamp to [-1, 1] in one launch
    (``ptmi_bigvgan_post``; bigvgan.py:349-351,380-385)."""
    _f32c(x, weight, bias)
    B, C, T = x.shape
    assert weight.dim() == 3 and weight.shape[:2] == (1, C) and (bias is None or bias.numel() == 1), (weight.shape, x.shape)
    out = torch.empty((B, 1, T), dtype=torch.float32, device=x.device)
    if out.numel():
        _lib.call('ptmi_bigvgan_post', x.data_ptr(), weight.data_ptr(), _lib.ptr(bias), B, C, T, weight.shape[2], int(tanh), out.data_ptr(),
                  _lib.stream(x.device), timer='bigvgan_post')
    return out


# ------------------------------------------------------------------------------------------------ attention (csrc/attention.hip)
def _attn_operand(t):
    """``[B, H, T, d]`` fp32 with a unit stride on ``d`` (any other strides: the projections' ``[B, T, H, d]`` output is read where it lies)."""
    assert t.dim() == 4 and t.dtype == torch.float32 and (t.stride(3) == 1 or t.shape[3] == 1), (t.shape, t.stride(), t.dtype)
    return t


def _attn_masks(lengths, mask, B, H, Tq, Tk):
    lengths, is64 = _lengths(lengths, B)
    strides = None
    if mask is not None:
        assert mask.dtype in (torch.uint8, torch.bool) and tuple(mask.shape) == (B, H, Tq, Tk), (mask.dtype, mask.shape, (B, H, Tq, Tk))
        strides = _lib.int64s(*mask.stride())
    return lengths, is64, mask, strides


def _attn_heads_last(B, H, T, d, device):
    """A contiguous ``[B, T, H, d]`` buffer, returned as its ``[B, H, T, d]`` view: what the ``out`` projection reads as ``[B T, H d]``."""
    return torch.empty((B, T, H, d), dtype=torch.float32, device=device).permute(0, 2, 1, 3)


@_register('attn_forward(Tensor q, Tensor k, Tensor v, Tensor? lengths, bool causal, Tensor? mask, float scale) -> (Tensor, Tensor)')
def attn_forward(q, k, v, lengths, causal, mask, scale):
    """``(out [B, H, Tq, dv] (a view of a contiguous [B, Tq, H, dv]), lse [B, H, Tq])`` (``ptmi_attn_forward``; transformer.py:28-38)."""
    B, H, Tq, dh = _attn_operand(q).shape
    Tk, dv = _attn_operand(k).shape[2], _attn_operand(v).shape[3]
    assert tuple(k.shape) == (B, H, Tk, dh) and tuple(v.shape) == (B, H, Tk, dv), (q.shape, k.shape, v.shape)
    lengths, is64, mask, mstr = _attn_masks(lengths, mask, B, H, Tq, Tk)
    out = _attn_heads_last(B, H, Tq, dv, q.device)
    lse = torch.empty((B, H, Tq), dtype=torch.float32, device=q.device)
    strides = _lib.int64s(*q.stride()[:3], *k.stride()[:3], *v.stride()[:3], *out.stride()[:3])
    _lib.call('ptmi_attn_forward', q.data_ptr(), k.data_ptr(), v.data_ptr(), strides, B, H, Tq, Tk, dh, dv, scale, _lib.ptr(lengths), is64,
              int(causal), _lib.ptr(mask), mstr, out.data_ptr(), lse.data_ptr(), _lib.stream(q.device), timer='attn_forward')
    return out, lse


@_register('attn_weights(Tensor q, Tensor k, Tensor lse, Tensor? lengths, bool causal, Tensor? mask, float scale) -> Tensor')
def attn_weights(q, k, lse, lengths, causal, mask, scale):
    """``softmax [B, H, Tq, Tk]`` from ``q``, ``k``, the forward's ``lse`` and the masks (``ptmi_attn_weights``)."""
    B, H, Tq, dh = _attn_operand(q).shape
    Tk = _attn_operand(k).shape[2]
    assert tuple(k.shape) == (B, H, Tk, dh) and tuple(lse.shape) == (B, H, Tq) and lse.is_contiguous(), (q.shape, k.shape, lse.shape)
    lengths, is64, mask, mstr = _attn_masks(lengths, mask, B, H, Tq, Tk)
    w = torch.empty((B, H, Tq, Tk), dtype=torch.float32, device=q.device)
    _lib.call('ptmi_attn_weights', q.data_ptr(), k.data_ptr(), lse.data_ptr(), _lib.int64s(*q.stride()[:3], *k.stride()[:3]), B, H, Tq, Tk, dh,
              scale, _lib.ptr(lengths), is64, int(causal), _lib.ptr(mask), mstr, w.data_ptr(), _lib.stream(q.device), timer='attn_weights')
    return w


@_register('attn_backward(Tensor q, Tensor k, Tensor v, Tensor out, Tensor dout, Tensor lse, Tensor? lengths, bool causal, Tensor? mask, '
           'float scale) -> (Tensor, Tensor, Tensor)')
def attn_backward(q, k, v, out, dout, lse, lengths, causal, mask, scale):
    """``(dq, dk, dv)`` as ``[B, H, T, d]`` views of contiguous ``[B, T, H, d]`` buffers (``ptmi_attn_backward``)."""
    B, H, Tq, dh = _attn_operand(q).shape
    Tk, dv = _attn_operand(k).shape[2], _attn_operand(v).shape[3]
    assert tuple(_attn_operand(out).shape) == (B, H, Tq, dv) and tuple(_attn_operand(dout).shape) == (B, H, Tq, dv), (out.shape, dout.shape)
    lengths, is64, mask, mstr = _attn_masks(lengths, mask, B, H, Tq, Tk)
    dev = q.device
    dq, dk, dvv = _attn_heads_last(B, H, Tq, dh, dev), _attn_heads_last(B, H, Tk, dh, dev), _attn_heads_last(B, H, Tk, dv, dev)
    delta = torch.empty((B, H, Tq), dtype=torch.float32, device=dev)
    strides = _lib.int64s(*[s for t in (q, k, v, out, dout, dq, dk, dvv) for s in t.stride()[:3]])
    _lib.call('ptmi_attn_backward', q.data_ptr(), k.data_ptr(), v.data_ptr(), out.data_ptr(), dout.data_ptr(), lse.data_ptr(), strides, B, H,
              Tq, Tk, dh, dv, scale, _lib.ptr(lengths), is64, int(causal), _lib.ptr(mask), mstr, delta.data_ptr(), dq.data_ptr(),
              dk.data_ptr(), dvv.data_ptr(), _lib.stream(dev), timer='attn_backward')
    return dq, dk, dvv


@_register('transformer_posenc_(Tensor(a!) x, Tensor freq) -> ()')
def transformer_posenc_(x, freq):
    """``x [B, T, d] += `` the interleaved cos / sin encoding with ``freq [d / 2] = 10000^(2i/d)``, in place (``ptmi_transformer_posenc``;
    transformer.py:234-243)."""
    _f32c(x, freq)
    B, T, d = x.shape
    assert d % 2 == 0 and freq.numel() == d // 2, (x.shape, freq.shape)
    _lib.call('ptmi_transformer_posenc', x.data_ptr(), x.data_ptr(), freq.data_ptr(), B, T, d, _lib.stream(x.device),
              timer='transformer_posenc')


@_register('transformer_norm_residual_forward(Tensor z, Tensor res, Tensor gamma, Tensor beta, Tensor? lengths, float eps, bool norm_first) '
           '-> (Tensor, Tensor?, Tensor)')
def transformer_norm_residual_forward(z, res, gamma, beta, lengths, eps, norm_first):
    """``(y, u or None, stats [B T, 2])`` of ``z, res [B, T, N]``: ``y = LN(z) + res`` (``norm_first``) or ``u = z + res``, ``y = LN(u)``
    (``ptmi_transformer_norm_residual_forward``; transformer.py:151-155)."""
    _f32c(z, res, gamma, beta)
    B, T, N = z.shape
    assert res.shape == z.shape and gamma.numel() == N and beta.numel() == N, (z.shape, res.shape, gamma.shape, beta.shape)
    lengths, is64 = _lengths(lengths, B)
    y = torch.empty_like(z)
    u = None if norm_first else torch.empty_like(z)
    stats = torch.empty((B * T, 2), dtype=torch.float32, device=z.device)
    _lib.call('ptmi_transformer_norm_residual_forward', z.data_ptr(), res.data_ptr(), gamma.data_ptr(), beta.data_ptr(), _lib.ptr(lengths),
              is64, B, T, N, eps, int(norm_first), y.data_ptr(), _lib.ptr(u), stats.data_ptr(), _lib.stream(z.device),
              timer='transformer_norm_residual_forward')
    return y, u, stats


@_register('transformer_norm_residual_backward(Tensor gy, Tensor v, Tensor stats, Tensor gamma, Tensor? lengths, bool want_params) '
           '-> (Tensor, Tensor?)')
def transformer_norm_residual_backward(gy, v, stats, gamma, lengths, want_params):
    """``(dv [B, T, N], dparams [2 N] = d gamma | d beta or None)`` for the normalised tensor ``v`` (``z``, or ``u`` when the norm came
    second) (``ptmi_transformer_norm_residual_backward``)."""
    lib = _lib.load()
    _f32c(gy, v, stats, gamma)
    B, T, N = v.shape
    assert gy.shape == v.shape and stats.shape == (B * T, 2) and gamma.numel() == N, (gy.shape, v.shape, stats.shape)
    lengths, is64 = _lengths(lengths, B)
    dv = torch.empty_like(v)
    dparams = torch.empty(2 * N, dtype=torch.float32, device=v.device) if want_params else None
    ws = _doubles(lib.ptmi_transformer_norm_workspace_elems(B * T, N), v.device) if want_params else None
    _lib.call('ptmi_transformer_norm_residual_backward', gy.data_ptr(), v.data_ptr(), stats.data_ptr(), gamma.data_ptr(), _lib.ptr(lengths),
              is64, B, T, N, dv.data_ptr(), _lib.ptr(dparams), _lib.ptr(ws), _lib.stream(v.device),
              timer='transformer_norm_residual_backward')
    return dv, dparams


# ------------------------------------------------------------------------------------------------ GRU + sequence glue (csrc/gru.hip, csrc/seq_pool.hip)
def _chunk_gru_dims(gates, table, H):
    _f32c(gates)
    _i32c(table)
    assert gates.dim() == 2 and table.dim() == 2 and table.shape[1] == 3 and gates.shape[1] % (3 * H) == 0, (gates.shape, table.shape, H)
    ndir = gates.shape[1] // (3 * H)
    assert ndir in (1, 2), gates.shape
    return gates.shape[0], ndir


@_register('chunk_gru_forward(Tensor(a!) gates, Tensor w_hh, Tensor? w_hh_reverse, Tensor? b_hh, Tensor? b_hh_reverse, Tensor table, '
           'int cap, int H, bool flip) -> (Tensor, Tensor)')
def chunk_gru_forward(gates, w_hh, w_hh_reverse, b_hh, b_hh_reverse, table, cap, H, flip):
    """The time loop of one GRU layer over the sequences of ``table [nseq, 3]``: ``gates [rows, ndir 3H]`` holds ``x W_ih^T + b_ih`` and
    becomes the activated ``(r, z, n)``; returns ``(h, q) [rows, ndir H]`` with ``q = h W_hn^T + b_hn`` (``ptmi_chunk_gru_forward``)."""
    rows, ndir = _chunk_gru_dims(gates, table, H)
    _f32c(w_hh, w_hh_reverse, b_hh, b_hh_reverse)
    assert w_hh.shape == (3 * H, H) and (ndir == 1 or w_hh_reverse.shape == (3 * H, H)), (w_hh.shape, ndir)
    assert all(b is None or b.shape == (3 * H,) for b in (b_hh, b_hh_reverse))
    h = torch.empty((rows, ndir * H), dtype=torch.float32, device=gates.device)
    q = torch.empty((rows, ndir * H), dtype=torch.float32, device=gates.device)
    rc = _lib.call('ptmi_chunk_gru_forward', gates.data_ptr(), w_hh.data_ptr(), _lib.ptr(w_hh_reverse), _lib.ptr(b_hh), _lib.ptr(b_hh_reverse),
                   q.data_ptr(), h.data_ptr(), table.data_ptr(), rows, table.shape[0], cap, H, ndir, int(flip), _lib.stream(gates.device),
                   timer=f'chunk_gru_forward:{table.shape[0]}x{cap}x{H}', accept=(-2,))
    if rc == -2:
        raise NotImplementedError(f'chunk_gru: hidden_size {H} is beyond the recurrence kernels\' bound')
    return h, q


@_register('chunk_gru_backward(Tensor(a!) gates, Tensor(b!) q, Tensor dh, Tensor w_hh, Tensor? w_hh_reverse, Tensor h, Tensor table, '
           'int cap, int H, bool flip) -> Tensor')
def chunk_gru_backward(gates, q, dh, w_hh, w_hh_reverse, h, table, cap, H, flip):
    """``gates`` becomes ``(dr_pre, dz_pre, dn_pre)``, ``q`` becomes ``dn_pre r``; returns ``hprev [rows, ndir H]``
    (``ptmi_chunk_gru_backward``)."""
    rows, ndir = _chunk_gru_dims(gates, table, H)
    _f32c(q, dh, w_hh, w_hh_reverse, h)
    assert dh.shape == h.shape == q.shape == (rows, ndir * H), (dh.shape, h.shape, q.shape)
    hprev = torch.empty_like(h)
    _lib.call('ptmi_chunk_gru_backward', gates.data_ptr(), q.data_ptr(), dh.data_ptr(), w_hh.data_ptr(), _lib.ptr(w_hh_reverse), h.data_ptr(),
              hprev.data_ptr(), table.data_ptr(), rows, table.shape[0], cap, H, ndir, int(flip), _lib.stream(gates.device),
              timer=f'chunk_gru_backward:{table.shape[0]}x{cap}x{H}')
    return hprev


@_register('seq_table(Tensor like, Tensor? lengths, int B, int T) -> Tensor')
def seq_table(like, lengths, B, T):
    """``table [B, 3]`` int32 = ``(b T, 1, clip(lengths[b], 0, T))`` on ``like``'s device; no lengths: ``T`` (``ptmi_seq_table``)."""
    lengths, is64 = _lengths(lengths, B)
    table = torch.empty((B, 3), dtype=torch.int32, device=like.device)
    _lib.call('ptmi_seq_table', _lib.ptr(lengths), is64, B, T, table.data_ptr(), _lib.stream(like.device), timer='seq_table')
    return table


@_register('seq_gather(Tensor x, Tensor? lengths, int mode) -> Tensor')
def seq_gather(x, lengths, mode):
    """``x [B, T, F]`` (any strides) -> contiguous ``[B, T, F]``: a copy (0), ``reverse_sequence`` (1) or its adjoint (2)
    (``ptmi_seq_gather``)."""
    assert x.dim() == 3 and x.dtype == torch.float32 and x.numel() > 0, (x.shape, x.dtype)
    B, T, F = x.shape
    lengths, is64 = _lengths(lengths, B)
    out = torch.empty((B, T, F), dtype=torch.float32, device=x.device)
    _lib.call('ptmi_seq_gather', x.data_ptr(), _lib.int64s(*x.stride()), _lib.ptr(lengths), is64, out.data_ptr(), B, T, F, mode,
              _lib.stream(x.device), timer='seq_gather')
    return out


@_register('seq_pool_forward(Tensor x, int[] dims, int[] strides, Tensor? lengths, int mode, Tensor? alpha, float alpha0, bool wave) '
           '-> (Tensor, Tensor?)')
def seq_pool_forward(x, dims, strides, lengths, mode, alpha, alpha0, wave):
    """``x`` read as ``[B, M, T, I] = dims`` through ``strides`` -> ``(y [B, M, I], index [B, M, I] int64 for mode 2)``
    (``ptmi_seq_pool_forward``)."""
    assert x.dtype == torch.float32 and len(dims) == 4 and len(strides) == 4 and min(dims) >= 1, (x.dtype, dims, strides)
    B, M, T, I = dims
    assert sum((d - 1) * s for d, s in zip(dims, strides)) < max(x.untyped_storage().nbytes() // 4 - x.storage_offset(), 1) and min(strides) >= 0
    lengths, is64 = _lengths(lengths, B)
    _f32c(alpha)
    assert alpha is None or (alpha.numel() == M and I == 1)
    y = torch.empty((B, M, I), dtype=torch.float32, device=x.device)
    index = torch.empty((B, M, I), dtype=torch.int64, device=x.device) if mode == 2 else None
    _lib.call('ptmi_seq_pool_forward', x.data_ptr(), _lib.int64s(*dims), _lib.int64s(*strides), _lib.ptr(lengths), is64, mode, _lib.ptr(alpha),
              alpha0, y.data_ptr(), _lib.ptr(index), int(wave), _lib.stream(x.device), timer=f'seq_pool_forward:{mode}')
    return y, index


@_register('seq_pool_backward(Tensor x, int[] dims, int[] strides, Tensor? lengths, int mode, Tensor? alpha, float alpha0, Tensor g, '
           'Tensor? y, Tensor? index, bool want_dalpha) -> (Tensor, Tensor?)')
def seq_pool_backward(x, dims, strides, lengths, mode, alpha, alpha0, g, y, index, want_dalpha):
    """``(dx [B, M, T, I] contiguous, dalpha [M] or None)`` (``ptmi_seq_pool_backward``); the thread map follows ``dx``'s layout: a
    wavefront per row when ``I == 1``."""
    assert x.dtype == torch.float32 and len(dims) == 4 and len(strides) == 4 and min(dims) >= 1, (x.dtype, dims, strides)
    B, M, T, I = dims
    lengths, is64 = _lengths(lengths, B)
    _f32c(alpha, g, y)
    assert g.numel() == B * M * I and (y is None or y.numel() == g.numel()) and (index is None or (index.numel() == g.numel()
                                                                                                   and index.is_contiguous()))
    dx = torch.empty((B, M, T, I), dtype=torch.float32, device=x.device)
    dalpha = ws = None
    if want_dalpha:
        assert mode == 4 and alpha is not None and I == 1
        dalpha = torch.empty(M, dtype=torch.float32, device=x.device)
        ws = _doubles(B * M, x.device)
    _lib.call('ptmi_seq_pool_backward', x.data_ptr(), _lib.int64s(*dims), _lib.int64s(*strides), _lib.ptr(lengths), is64, mode,
              _lib.ptr(alpha), alpha0, g.data_ptr(), _lib.ptr(y), _lib.ptr(index), dx.data_ptr(), _lib.ptr(ws), _lib.ptr(dalpha), int(I == 1),
              _lib.stream(x.device), timer=f'seq_pool_backward:{mode}')
    return dx, dalpha


# ------------------------------------------------------------------------------------------------ contrib/je convolution blocks (csrc/je_conv.hip)
#: the activation codes of ptmi_je_conv_*
JE_CONV_ACTIVATIONS = {'identity': 0, 'relu': 1, 'leaky_relu': 2, 'elu': 3, 'tanh': 4, 'sigmoid': 5, 'prelu': 6}


def _jc_rows(t, width, what):
    """``t [rows, width]`` as (pointer, row stride): unit inner stride."""
    assert t.dim() == 2 and t.dtype == torch.float32 and t.shape[1] == width and (t.stride(1) == 1 or width == 1), (what, t.shape, t.stride())
    return t.data_ptr(), max(_ld(t), width)


@_register('je_conv_taps(Tensor P, Tensor? bias, Tensor? gate_bias, Tensor? residual, Tensor? slope, int[] geom, int act, float act_p, '
           'bool fused) -> (Tensor, Tensor?, Tensor?)')
def je_conv_taps(P, bias, gate_bias, residual, slope, geom, act, act_p, fused):
    """``(z, gz or None, out or None) [B T_out, C_out]`` from ``P [B T_in, G K C_out]``; ``geom = (B, T_in, T_out, C_out, K, stride,
    dilation, front, G)``; ``fused``: the epilogue ``out = act(z) sigmoid(gz) + residual`` in the same launch (``ptmi_je_conv_taps``)."""
    _f32c(P, bias, gate_bias, slope)
    B, T_in, T_out, C_out, K, _, _, _, G = geom
    assert tuple(P.shape) == (B * T_in, G * K * C_out), (P.shape, geom)
    assert all(b is None or b.numel() == C_out for b in (bias, gate_bias))
    rp, ldr = (None, C_out) if residual is None else _jc_rows(residual, C_out, 'residual')
    assert residual is None or residual.shape[0] == B * T_out
    dev = P.device
    z = torch.empty((B * T_out, C_out), dtype=torch.float32, device=dev)
    gz = torch.empty_like(z) if G == 2 else None
    out = torch.empty_like(z) if fused else None
    _lib.call('ptmi_je_conv_taps', P.data_ptr(), _lib.ptr(bias), _lib.ptr(gate_bias), rp, _lib.ptr(slope), z.data_ptr(), _lib.ptr(gz),
              _lib.ptr(out), _lib.int64s(*geom, G * K * C_out, ldr), act, act_p, _lib.stream(dev), timer='je_conv_taps')
    return z, gz, out


@_register('je_conv_dtaps(Tensor dz, Tensor? dgz, int[] geom) -> Tensor')
def je_conv_dtaps(dz, dgz, geom):
    """``dP [B T_in, G K C_out]`` in gather form from ``dz`` / ``dgz [B T_out, C_out]`` (``ptmi_je_conv_dtaps``)."""
    _f32c(dz, dgz)
    B, T_in, T_out, C_out, K, _, _, _, G = geom
    assert tuple(dz.shape) == (B * T_out, C_out) and (G == 1 or dgz.shape == dz.shape), (dz.shape, geom)
    dP = torch.empty((B * T_in, G * K * C_out), dtype=torch.float32, device=dz.device)
    _lib.call('ptmi_je_conv_dtaps', dz.data_ptr(), _lib.ptr(dgz), dP.data_ptr(), _lib.int64s(*geom, G * K * C_out, C_out),
              _lib.stream(dz.device), timer='je_conv_dtaps')
    return dP


@_register('je_conv_stats(Tensor x, Tensor? lengths, int B, int T, bool per_example, float eps) -> Tensor')
def je_conv_stats(x, lengths, B, T, per_example, eps):
    """``stats [groups, 4, C]`` = mean, rstd, power, count of ``x [B T, C]`` over ``t < lengths[b]`` (``ptmi_je_conv_stats``)."""
    C = x.shape[1]
    xp, ldx = _jc_rows(x, C, 'x')
    assert x.shape[0] == B * T
    lengths, is64 = _lengths(lengths, B)
    groups = B if per_example else 1
    ws = _doubles(_lib.load().ptmi_je_conv_workspace_elems(B, T, C), x.device)
    sums = _doubles(3 * groups * C, x.device)
    stats = torch.empty((groups, 4, C), dtype=torch.float32, device=x.device)
    _lib.call('ptmi_je_conv_stats', xp, ldx, _lib.ptr(lengths), is64, B, T, C, int(per_example), eps, ws.data_ptr(), sums.data_ptr(),
              stats.data_ptr(), _lib.stream(x.device), timer='je_conv_stats')
    return stats


@_register('je_conv_apply(Tensor z, Tensor? g, Tensor? residual, Tensor? stats, Tensor? gamma, Tensor? beta, Tensor? lengths, '
           'Tensor? slope, int B, int T, bool per_example, int act, float act_p) -> Tensor')
def je_conv_apply(z, g, residual, stats, gamma, beta, lengths, slope, B, T, per_example, act, act_p):
    """``out [B T, C] = act(n) sigmoid(g) + residual``, ``n = gamma (z - mean) rstd + beta`` and 0 behind the length (``ptmi_je_conv_apply``)."""
    C = z.shape[1]
    zp, ldz = _jc_rows(z, C, 'z')
    rp, ldr = (None, C) if residual is None else _jc_rows(residual, C, 'residual')
    _f32c(g, stats, gamma, beta, slope)
    assert z.shape[0] == B * T and (g is None or g.shape == z.shape) and (residual is None or residual.shape == z.shape)
    assert stats is None or tuple(stats.shape) == (B if per_example else 1, 4, C), (stats.shape, B, C)
    assert all(p is None or p.numel() == C for p in (gamma, beta))
    lengths, is64 = _lengths(lengths, B)
    out = torch.empty((B * T, C), dtype=torch.float32, device=z.device)
    _lib.call('ptmi_je_conv_apply', zp, ldz, _lib.ptr(g), rp, ldr, _lib.ptr(stats), _lib.ptr(gamma), _lib.ptr(beta), _lib.ptr(lengths), is64,
              _lib.ptr(slope), out.data_ptr(), B, T, C, int(per_example), act, act_p, _lib.stream(z.device), timer='je_conv_apply')
    return out


@_register('je_conv_apply_backward(Tensor dout, Tensor z, Tensor? g, Tensor? stats, Tensor? gamma, Tensor? beta, Tensor? lengths, '
           'Tensor? slope, int B, int T, bool per_example, bool fixed_stats, int act, float act_p, bool want_params) '
           '-> (Tensor, Tensor?, Tensor?)')
def je_conv_apply_backward(dout, z, g, stats, gamma, beta, lengths, slope, B, T, per_example, fixed_stats, act, act_p, want_params):
    """``(dz, dgz or None, dparams [2 C + 1] = d gamma | d beta | d slope or None)`` (``ptmi_je_conv_apply_backward``)."""
    C = z.shape[1]
    zp, ldz = _jc_rows(z, C, 'z')
    _f32c(dout, g, stats, gamma, beta, slope)
    assert dout.shape == z.shape and z.shape[0] == B * T and (g is None or g.shape == z.shape)
    assert stats is None or tuple(stats.shape) == (B if per_example else 1, 4, C), (stats.shape, B, C)
    lengths, is64 = _lengths(lengths, B)
    dev = z.device
    dz = torch.empty((B * T, C), dtype=torch.float32, device=dev)
    dgz = torch.empty_like(dz) if g is not None else None
    dparams = torch.empty(2 * C + 1, dtype=torch.float32, device=dev) if want_params else None
    ws = sums = None
    if want_params or (stats is not None and not fixed_stats):
        ws = _doubles(_lib.load().ptmi_je_conv_workspace_elems(B, T, C), dev)
        sums = _doubles(3 * (B if per_example and stats is not None else 1) * C, dev)
    _lib.call('ptmi_je_conv_apply_backward', dout.data_ptr(), zp, ldz, _lib.ptr(g), _lib.ptr(stats), _lib.ptr(gamma), _lib.ptr(beta),
              _lib.ptr(lengths), is64, _lib.ptr(slope), dz.data_ptr(), _lib.ptr(dgz), _lib.ptr(dparams), _lib.ptr(ws), _lib.ptr(sums), B, T, C,
              int(per_example), int(fixed_stats), act, act_p, _lib.stream(dev), timer='je_conv_apply_backward')
    return dz, dgz, dparams


@_register('je_pool_forward(Tensor x, int[] geom, bool max_pool) -> (Tensor, Tensor?)')
def je_pool_forward(x, geom, max_pool):
    """``(y [B T_out, C], index int64 or None)`` from ``x [B T_in, C]``; ``geom = (B, T_in, T_out, C, size, stride, front)``
    (``ptmi_je_pool_forward``)."""
    B, T_in, T_out, C = geom[:4]
    xp, ldx = _jc_rows(x, C, 'x')
    assert x.shape[0] == B * T_in
    y = torch.empty((B * T_out, C), dtype=torch.float32, device=x.device)
    index = torch.empty((B * T_out, C), dtype=torch.int64, device=x.device) if max_pool else None
    _lib.call('ptmi_je_pool_forward', xp, y.data_ptr(), _lib.ptr(index), _lib.int64s(*geom, ldx), int(max_pool), _lib.stream(x.device),
              timer='je_pool_forward')
    return y, index


@_register('je_pool_backward(Tensor dy, Tensor? index, int[] geom, bool max_pool) -> Tensor')
def je_pool_backward(dy, index, geom, max_pool):
    """``dx [B T_in, C]`` (``ptmi_je_pool_backward``)."""
    B, T_in, T_out, C = geom[:4]
    _f32c(dy)
    assert tuple(dy.shape) == (B * T_out, C) and (index is None or (index.shape == dy.shape and index.is_contiguous() and index.dtype == torch.int64))
    dx = torch.empty((B * T_in, C), dtype=torch.float32, device=dy.device)
    _lib.call('ptmi_je_pool_backward', dy.data_ptr(), _lib.ptr(index), dx.data_ptr(), _lib.int64s(*geom, C), int(max_pool),
              _lib.stream(dy.device), timer='je_pool_backward')
    return dx
