"""The dual-path RNN (``padertorch/modules/dual_path_rnn.py``) on the HIP kernels of ``csrc/dprnn.hip`` and the split-fp16 GEMM.

The chunked activation is ``[B, S, K, N]`` (channels last, chunk-major) from :func:`segment_rows` to :func:`overlap_add_rows`; its rows
``(b, s, k)`` are "positions".  Both paths of a block walk the SAME buffer through a sequence table ``[nseq, 3]`` = (base row, step
stride, step count): intra-chunk sequences have stride 1, inter-chunk sequences stride ``K``.  Nothing is transposed or copied.

    num_chunks(L, K, P), chunk_counts(lengths, K, P)       the reference's S and S_b (host arithmetic)
    tables(like, lengths, B, S, K, P)                      (chunks [B], intra [B S, 3], inter [B K, 3]) in device memory, no synchronisation
    segment_rows(x [B, L, N], K, P) -> [B, S, K, N]        differentiable; each is the other's backward
    overlap_add_rows(seg [B, S, K, N], P) -> [B, S P - (K - P), N]
    chunk_lstm(x [rows, N], table, cap, rnn) -> [rows, D H] one ``torch.nn.LSTM`` layer over the table's sequences
    chunk_lstm_params(x [rows, N], table, cap, w_ih, w_hh, b_ih, b_hh, ...) -> [rows, D H]   the same for one layer's parameter tensors
    chunk_rnn(x [rows, N], table, cap, chunks, S, K, rnn, fc, norm) -> [rows, N]
        one ``_ChunkRNN``: LSTM, projection, layer norm (zeros on the positions with ``s >= chunks[b]``), plus ``x``

The input projection, ``fc`` and every weight gradient are calls of ``ops.gemm.mm``; the kernels do the time loop, the norm and the sums
over rows.  fp32 on the GPU only: other dtypes raise ``NotImplementedError``, CPU tensors the "no CPU fallback"
error.
"""
import torch
from torch.autograd.function import once_differentiable

from .. import _lib
from . import gemm as _gemm
from . import library  # noqa: F401  (registers torch.ops.ptmi.*)

__all__ = ['num_chunks', 'chunk_counts', 'tables', 'segment_rows', 'overlap_add_rows', 'chunk_lstm', 'chunk_lstm_params', 'chunk_rnn', 'MAX_HIDDEN', 'RESIDENT_HIDDEN']

#: the largest ``hidden_size`` the recurrence kernels take (``ptmi_chunk_lstm_max_hidden``); up to :data:`RESIDENT_HIDDEN` ``W_hh`` stays
#: in the registers of a workgroup, above it is streamed from the L2 every step
MAX_HIDDEN = 1536
RESIDENT_HIDDEN = 128


def _check(name, *tensors):
    for t in tensors:
        if t is not None and t.dtype != torch.float32:
            raise NotImplementedError(f'{name}: float32 only, got {t.dtype}')
    _lib.require_gpu(*tensors)


def num_chunks(L, K, P):
    """Chunks ``S`` of a signal of ``L`` frames: ``K - P`` zero frames in front and behind, windows of ``K`` every ``P``, the last one
    padded (``dual_path_rnn.py:139-143``)."""
    padded = L + 2 * (K - P)
    return 1 if padded <= K else -(-(padded - K) // P) + 1


def chunk_counts(lengths, K, P):
    """``S_b``: the chunks that hold a part of an example of ``lengths[b]`` frames (``dual_path_rnn.py:146-149``), for a tensor or a
    list; the kernels compute the same on the device."""
    if not torch.is_tensor(lengths):
        lengths = torch.tensor(lengths)
    return torch.div(lengths + (K - P) - 1, P, rounding_mode='floor') + 1


def tables(like, lengths, B, S, K, P):
    """``(chunks [B], intra [B S, 3], inter [B K, 3])`` int32 on ``like``'s device.  ``lengths``: ``[B]`` frames as an int32 / int64
    tensor (on the GPU it is read by the kernel: a captured graph serves any pattern; a CPU tensor or a list is copied there without a
    synchronisation) or None (every chunk counts)."""
    _lib.require_gpu(like)
    if lengths is not None:
        if not torch.is_tensor(lengths):
            lengths = [int(n) for n in lengths]
        if not (torch.is_tensor(lengths) and lengths.is_cuda):
            lengths = _lib.host_to_device(lengths, torch.int64, like.device)
        lengths = lengths.reshape(-1)
        if lengths.dtype not in (torch.int32, torch.int64) or lengths.numel() != B:
            raise ValueError(f'dprnn: sequence_lengths [{B}] int32 or int64, got {lengths.dtype} {tuple(lengths.shape)}')
        lengths = lengths.to(like.device).contiguous()
    return torch.ops.ptmi.dprnn_tables(like, lengths, B, S, K, P)


class _SegmentFn(torch.autograd.Function):
    """Kernel ``dprnn_segment``; backward: ``dprnn_overlap_add`` of the gradient, cut to the input's frames."""

    @staticmethod
    def forward(ctx, x, K, P):
        ctx.dims = (x.shape[1], K, P)
        return torch.ops.ptmi.dprnn_segment(x, K, P)

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        L, K, P = ctx.dims
        return torch.ops.ptmi.dprnn_overlap_add(g, P, L, K - P), None, None


class _OverlapAddFn(torch.autograd.Function):
    """Kernel ``dprnn_overlap_add`` over the whole unpadded length ``S P - (K - P)``; backward: ``dprnn_segment`` of the gradient, which
    has exactly ``S`` chunks again."""

    @staticmethod
    def forward(ctx, seg, P):
        B, S, K, N = seg.shape
        ctx.dims = (S, K, P)
        return torch.ops.ptmi.dprnn_overlap_add(seg, P, S * P - (K - P), K - P)

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        S, K, P = ctx.dims
        seg = torch.ops.ptmi.dprnn_segment(g, K, P)
        assert seg.shape[1] == S, (seg.shape, S)
        return seg, None


def _geometry(name, K, P):
    K, P = int(K), int(P)
    if not 1 <= P <= K:
        raise ValueError(f'{name}: 1 <= hop_size <= window_size, got hop_size {P}, window_size {K}')
    return K, P


def segment_rows(x, K, P):
    """``x [B, L, N]`` (any strides) -> ``[B, S, K, N]``, ``S = num_chunks(L, K, P)``: ``seg[b, s, k] = x[b, s P + k - (K - P)]``, zeros
    outside the signal."""
    _check('segment_rows', x)
    K, P = _geometry('segment_rows', K, P)
    if x.dim() != 3 or x.numel() == 0:
        raise ValueError(f'segment_rows: x [B, L, N], got {tuple(x.shape)}')
    return _SegmentFn.apply(x, K, P)


def overlap_add_rows(seg, P):
    """``seg [B, S, K, N]`` (any strides) -> ``[B, S P - (K - P), N]``, the reference's unpadded length: every frame is the sum, chunks
    ascending, of the elements :func:`segment_rows` copies it to."""
    _check('overlap_add_rows', seg)
    if seg.dim() != 4 or seg.numel() == 0:
        raise ValueError(f'overlap_add_rows: seg [B, S, K, N], got {tuple(seg.shape)}')
    K, P = _geometry('overlap_add_rows', seg.shape[2], P)
    if seg.shape[1] * P - (K - P) < 1:
        raise ValueError(f'overlap_add_rows: no frame is left of {seg.shape[1]} chunks of {K} frames every {P}')
    return _OverlapAddFn.apply(seg, P)


# ---------------------------------------------------------------------------------------------------- the LSTM layer
def _directions(params):
    """``params``: (w_ih, w_hh, b_ih, b_hh) per direction, flat; None entries close the list."""
    return [params[i:i + 4] for i in range(0, len(params), 4) if params[i] is not None]


def _lstm_forward(x, table, cap, dirs):
    """``x [rows, N]`` -> ``(gates [rows, D 4H] activated, h, c [rows, D H])``: one GEMM per direction into its column block of
    ``gates`` (``b_ih`` by the GEMM's epilogue), then the recurrence kernel (which adds ``b_hh``)."""
    H = dirs[0][1].shape[1]
    D = len(dirs)
    gates = torch.empty((x.shape[0], D * 4 * H), dtype=torch.float32, device=x.device)
    for d, (w_ih, _, b_ih, _) in enumerate(dirs):
        _gemm.mm(x, w_ih.t(), bias=b_ih, out=gates[:, d * 4 * H:(d + 1) * 4 * H])
    rev = dirs[1] if D == 2 else (None,) * 4
    h, c = torch.ops.ptmi.chunk_lstm_forward(gates, dirs[0][1], rev[1], dirs[0][3], rev[3], table, cap, H)
    return gates, h, c


def _lstm_backward(dh, x, gates, h, c, table, cap, dirs, dx_out, need_dx):
    """The reverse time loop (``gates`` becomes ``d gates``) and the GEMMs of ``dW_ih``, ``dW_hh`` and ``dx``; the bias gradients are
    column sums of ``d gates``.  ``dx_out``: a buffer the input gradient is ADDED to, or None.  Returns ``(dx, [dw_ih, dw_hh, db_ih,
    db_hh] per direction)``."""
    H = dirs[0][1].shape[1]
    D = len(dirs)
    rev = dirs[1] if D == 2 else (None,) * 4
    hprev = torch.ops.ptmi.chunk_lstm_backward(gates, dh, dirs[0][1], rev[1], h, c, table, cap, H)
    db_ih, db_hh = torch.ops.ptmi.dprnn_colsum_pair(gates)          # one pass over the rows, two tensors: two parameters
    grads, dx = [], dx_out
    for d, (w_ih, _, _, _) in enumerate(dirs):
        dg = gates[:, d * 4 * H:(d + 1) * 4 * H]
        grads += [_gemm.mm(dg.t(), x), _gemm.mm(dg.t(), hprev[:, d * H:(d + 1) * H]),
                  db_ih[d * 4 * H:(d + 1) * 4 * H], db_hh[d * 4 * H:(d + 1) * 4 * H]]
        if need_dx:
            dx = _gemm.mm(dg, w_ih) if dx is None else _gemm.mm(dg, w_ih, out=dx, accumulate=True)
    return dx, grads


def _spent(ctx):
    if getattr(ctx, 'spent', False):
        raise RuntimeError('dprnn: the backward pass overwrites the saved gates with their gradient and runs once per forward; '
                           'run the forward again instead of retain_graph=True')
    ctx.spent = True


class _ChunkLstmFn(torch.autograd.Function):
    """GEMMs and ``chunk_lstm_forward``; ``chunk_lstm_backward`` and GEMMs.  Saves ``x``, the activated gates, ``h`` and ``c``."""

    @staticmethod
    def forward(ctx, x, table, cap, *params):
        dirs = _directions(params)
        gates, h, c = _lstm_forward(x, table, cap, dirs)
        ctx.save_for_backward(x, table, h, c, *params)
        ctx.gates, ctx.cap = gates, cap
        return h

    @staticmethod
    @once_differentiable
    def backward(ctx, dh):
        _spent(ctx)
        x, table, h, c, *params = ctx.saved_tensors
        dirs = _directions(params)
        dx, grads = _lstm_backward(dh.contiguous(), x, ctx.gates, h, c, table, ctx.cap, dirs, None, ctx.needs_input_grad[0])
        ctx.gates = None
        grads += [None] * (len(params) - len(grads))
        return (dx, None, None, *[g if need else None for g, need in zip(grads, ctx.needs_input_grad[3:])])


class _ChunkRnnFn(torch.autograd.Function):
    """One ``_ChunkRNN`` as ONE node, so that the two gradients of its input (through the LSTM and through the residual) are added by
    the last GEMM's epilogue and not by a kernel of autograd: ``_lstm_forward``, the projection GEMM, ``dprnn_norm_residual_forward``;
    ``dprnn_norm_residual_backward``, the projection's three gradients, ``_lstm_backward``."""

    @staticmethod
    def forward(ctx, x, table, chunks, cap, S, K, eps, fc_w, fc_b, gamma, beta, *params):
        dirs = _directions(params)
        gates, h, c = _lstm_forward(x, table, cap, dirs)
        z = _gemm.mm(h, fc_w.t(), bias=fc_b)
        y, stats = torch.ops.ptmi.dprnn_norm_residual_forward(z, x, gamma, beta, chunks, S, K, eps)
        ctx.save_for_backward(x, table, chunks, h, c, z, stats, fc_w, gamma, *params)
        ctx.gates, ctx.dims = gates, (cap, S, K)
        return y

    @staticmethod
    @once_differentiable
    def backward(ctx, gy):
        _spent(ctx)
        x, table, chunks, h, c, z, stats, fc_w, gamma, *params = ctx.saved_tensors
        cap, S, K = ctx.dims
        dirs = _directions(params)
        need = ctx.needs_input_grad
        dz, dres, dparams = torch.ops.ptmi.dprnn_norm_residual_backward(gy.contiguous(), z, stats, gamma, chunks, S, K)
        n = gamma.numel()
        d_fc_w = _gemm.mm(dz.t(), h) if need[7] else None
        d_fc_b = torch.ops.ptmi.dprnn_colsum(dz) if need[8] else None
        dh = _gemm.mm(dz, fc_w)
        dx, grads = _lstm_backward(dh, x, ctx.gates, h, c, table, cap, dirs, dres, need[0])
        ctx.gates = None
        grads += [None] * (len(params) - len(grads))
        return (dx if need[0] else None, None, None, None, None, None, None, d_fc_w, d_fc_b,
                dparams[:n] if need[9] else None, dparams[n:] if need[10] else None,
                *[g if nd else None for g, nd in zip(grads, need[11:])])


def _rnn_params(name, rnn):
    if not isinstance(rnn, torch.nn.LSTM) or rnn.num_layers != 1 or not rnn.bias or rnn.proj_size != 0:
        raise NotImplementedError(f'{name}: a torch.nn.LSTM of one layer with biases and without projection, got {rnn!r}')
    if rnn.hidden_size > MAX_HIDDEN:
        raise NotImplementedError(f'{name}: hidden_size {rnn.hidden_size} > {MAX_HIDDEN}: the recurrence kernels keep the gate '
                                  f'gradients, dh and dc of a tile of four sequences in LDS: 96 bytes per unit of the 160 KB of a CU')
    params = [rnn.weight_ih_l0, rnn.weight_hh_l0, rnn.bias_ih_l0, rnn.bias_hh_l0]
    if rnn.bidirectional:
        params += [rnn.weight_ih_l0_reverse, rnn.weight_hh_l0_reverse, rnn.bias_ih_l0_reverse, rnn.bias_hh_l0_reverse]
    else:
        params += [None] * 4
    return params


def _table(name, x, table, cap):
    if x.dim() != 2 or x.numel() == 0 or not x.is_contiguous():
        raise ValueError(f'{name}: x [rows, N] contiguous, got {tuple(x.shape)} with strides {x.stride()}')
    if table.dtype != torch.int32 or table.dim() != 2 or table.shape[1] != 3 or table.shape[0] < 1 or not table.is_cuda:
        raise ValueError(f'{name}: table [nseq, 3] int32 on the GPU, got {table.dtype} {tuple(table.shape)} on {table.device}')
    if int(cap) < 1:
        raise ValueError(f'{name}: cap >= 1, got {cap}')
    return table.contiguous(), int(cap)


def chunk_lstm(x, table, cap, rnn):
    """``x [rows, N]`` -> ``h [rows, D H]``: the layer ``rnn`` (``torch.nn.LSTM``, uni- or bidirectional, zero initial state) over the
    sequences of ``table [nseq, 3]`` int32 = (base row, step stride, step count <= cap).  Sequence ``i`` occupies the rows ``base_i + t
    stride_i``, ``t < cap``, which must lie inside ``x`` and belong to no other sequence; its steps are the first ``count_i`` of them, the
    reverse direction starts at the last of THOSE (PackedSequence semantics), and ``h`` is zero on the others.  EVERY row of ``x`` must
    belong to a sequence: the GEMMs of the weight gradients read all rows, and only the table's rows are written."""
    _check('chunk_lstm', x)
    table, cap = _table('chunk_lstm', x, table, cap)
    params = _rnn_params('chunk_lstm', rnn)
    if x.shape[1] != rnn.input_size:
        raise ValueError(f'chunk_lstm: x [rows, {rnn.input_size}], got {tuple(x.shape)}')
    _check('chunk_lstm', *params)
    return _ChunkLstmFn.apply(x, table, cap, *params)


def chunk_lstm_params(x, table, cap, w_ih, w_hh, b_ih, b_hh, w_ih_reverse=None, w_hh_reverse=None, b_ih_reverse=None,
                      b_hh_reverse=None):
    """:func:`chunk_lstm` for the parameter tensors of ONE layer (``weight_ih [4H, N]``, ``weight_hh [4H, H]``, ``bias_ih``, ``bias_hh
    [4H]``; the ``_reverse`` four make it bidirectional), so that a multi-layer ``torch.nn.LSTM`` can be walked layer by layer."""
    params = [w_ih, w_hh, b_ih, b_hh, w_ih_reverse, w_hh_reverse, b_ih_reverse, b_hh_reverse]
    _check('chunk_lstm', x, *params)
    table, cap = _table('chunk_lstm', x, table, cap)
    dirs = _directions(params)
    if not dirs or any(p is None for d in dirs for p in d):
        raise NotImplementedError('chunk_lstm: weight_ih, weight_hh, bias_ih and bias_hh per direction (the recurrence kernel has no '
                                  'bias-free form)')
    H = w_hh.shape[1]
    for w_i, w_h, b_i, b_h in dirs:
        if tuple(w_i.shape) != (4 * H, x.shape[1]) or tuple(w_h.shape) != (4 * H, H) or b_i.shape != (4 * H,) or b_h.shape != (4 * H,):
            raise ValueError(f'chunk_lstm: weight_ih [{4 * H}, {x.shape[1]}], weight_hh [{4 * H}, {H}] and biases [{4 * H}], got '
                             f'{tuple(w_i.shape)}, {tuple(w_h.shape)}, {tuple(b_i.shape)}, {tuple(b_h.shape)}')
    if H > MAX_HIDDEN:
        raise NotImplementedError(f'chunk_lstm: hidden_size {H} > {MAX_HIDDEN}')
    if len(dirs) == 1:
        params[4:] = [None] * 4
    return _ChunkLstmFn.apply(x, table, cap, *params)


def chunk_rnn(x, table, cap, chunks, S, K, rnn, fc, norm):
    """One ``_ChunkRNN`` (``dual_path_rnn.py:428-499``) on the rows ``x [B S K, N]`` of the chunked activation: ``y = mask(norm(fc(lstm(x))))
    + x`` with the LSTM over the sequences of ``table`` (:func:`chunk_lstm`) and ``mask`` = zeros on the positions ``(b, s, k)`` with ``s >=
    chunks[b]`` (``chunks`` None: none)."""
    _check('chunk_rnn', x)
    table, cap = _table('chunk_rnn', x, table, cap)
    params = _rnn_params('chunk_rnn', rnn)
    N = x.shape[1]
    if rnn.input_size != N or fc.out_features != N or fc.bias is None or tuple(norm.normalized_shape) != (N,) or norm.weight is None:
        raise ValueError(f'chunk_rnn: an LSTM, a Linear with bias and an affine LayerNorm of feature size {N}')
    if x.shape[0] % (S * K) != 0:
        raise ValueError(f'chunk_rnn: rows = B S K, got {x.shape[0]} rows with S = {S}, K = {K}')
    _check('chunk_rnn', fc.weight, fc.bias, norm.weight, norm.bias, *params)
    return _ChunkRnnFn.apply(x, table, chunks, cap, int(S), int(K), float(norm.eps), fc.weight, fc.bias, norm.weight, norm.bias, *params)
