"""One ``torch.nn.GRU`` layer over a table of sequences on the recurrence kernels of ``csrc/gru.hip`` and the split-fp16 GEMM.

    sequence_table(like, seq_len, B, T) -> [B, 3] int32      (b T, 1, len_b) of a padded batch ``[B, T, .]``, built on the device
    chunk_gru(x [rows, N], table, cap, w_ih, w_hh, b_ih, b_hh, (the reverse direction's four), flip=False) -> h [rows, D H]

The contract is :func:`ops.dprnn.chunk_lstm`'s: sequence ``i`` occupies the rows ``base_i + t stride_i``, ``t < cap``, its steps are the
first ``count_i`` of them, ``h`` is zero on the others, the reverse direction starts at the sequence's own last step, and EVERY row of
``x`` belongs to exactly one sequence (the weight-gradient GEMMs read all rows).  The initial state is zero, the final state is not
returned.  ``flip=True`` runs direction ``d`` in the opposite sense of time.

The input projection is one ``ops.gemm.mm`` per direction into its column block of a ``[rows, D 3H]`` buffer; the kernels do the time
loop; ``dW_ih``, ``dW_hh`` and ``dx`` are ``ops.gemm.mm`` calls over the two gradient operands the backward kernel writes, the bias
gradients ordered fp64 column sums.  fp32 on the GPU only: other dtypes raise ``NotImplementedError``, CPU tensors the
"no CPU fallback" error.
"""
import torch
from torch.autograd.function import once_differentiable

from .. import _lib
from . import gemm as _gemm
from . import library  # noqa: F401  (registers torch.ops.ptmi.*)

__all__ = ['chunk_gru', 'sequence_table', 'device_lengths', 'MAX_HIDDEN', 'RESIDENT_HIDDEN']

#: the largest ``hidden_size`` the recurrence kernels take (``ptmi_chunk_gru_max_hidden``): the streamed backward kernel keeps the
#: ``W_hh`` operand (3 H), the recurrent part of ``dh`` and the carried ``dh z`` of a tile of four sequences in LDS, 80 bytes per unit
MAX_HIDDEN = 1792
RESIDENT_HIDDEN = 128


def _check(name, *tensors):
    for t in tensors:
        if t is not None and t.dtype != torch.float32:
            raise NotImplementedError(f'{name}: float32 only, got {t.dtype}')
    _lib.require_gpu(*tensors)


def device_lengths(seq_len, B, device):
    """``seq_len`` (None, list, numpy array, CPU or CUDA tensor) as a contiguous int32 / int64 CUDA vector ``[B]``; host forms are copied
    without a synchronisation."""
    if seq_len is None:
        return None
    if not (torch.is_tensor(seq_len) and seq_len.is_cuda):
        if torch.is_tensor(seq_len):
            seq_len = seq_len.detach().reshape(-1).to(torch.int64)
        else:
            seq_len = [int(n) for n in seq_len]
        seq_len = _lib.host_to_device(seq_len, torch.int64, device)
    seq_len = seq_len.reshape(-1)
    if seq_len.dtype not in (torch.int32, torch.int64) or seq_len.numel() != B:
        raise ValueError(f'seq_len [{B}] int32 or int64, got {seq_len.dtype} {tuple(seq_len.shape)}')
    return seq_len.contiguous()


def sequence_table(like, seq_len, B, T):
    """``[B, 3]`` int32 = ``(b T, 1, clip(len_b, 0, T))`` on ``like``'s device (``seq_len`` None: ``T`` steps each)."""
    _lib.require_gpu(like)
    return torch.ops.ptmi.seq_table(like, device_lengths(seq_len, B, like.device), int(B), int(T))


def _directions(params):
    return [params[i:i + 4] for i in range(0, 8, 4) if params[i] is not None]


def _spent(ctx):
    if getattr(ctx, 'spent', False):
        raise RuntimeError('chunk_gru: the backward pass overwrites the saved gates with their gradient and runs once per forward; '
                           'run the forward again instead of retain_graph=True')
    ctx.spent = True


class _ChunkGruFn(torch.autograd.Function):
    """GEMMs and ``chunk_gru_forward``; ``chunk_gru_backward`` and GEMMs.  Saves ``x``, ``h``, the activated gates and ``q``."""

    @staticmethod
    def forward(ctx, x, table, cap, flip, *params):
        dirs = _directions(params)
        H, D = dirs[0][1].shape[1], len(dirs)
        gates = torch.empty((x.shape[0], D * 3 * H), dtype=torch.float32, device=x.device)
        for d, (w_ih, _, b_ih, _) in enumerate(dirs):
            _gemm.mm(x, w_ih.t(), bias=b_ih, out=gates[:, d * 3 * H:(d + 1) * 3 * H])
        rev = dirs[1] if D == 2 else (None,) * 4
        h, q = torch.ops.ptmi.chunk_gru_forward(gates, dirs[0][1], rev[1], dirs[0][3], rev[3], table, cap, H, flip)
        ctx.save_for_backward(x, table, h, *params)
        ctx.gates, ctx.q, ctx.cfg = gates, q, (cap, flip)
        return h

    @staticmethod
    @once_differentiable
    def backward(ctx, dh):
        _spent(ctx)
        x, table, h, *params = ctx.saved_tensors
        cap, flip = ctx.cfg
        dirs = _directions(params)
        H, D = dirs[0][1].shape[1], len(dirs)
        gates, q = ctx.gates, ctx.q
        ctx.gates = ctx.q = None
        rev = dirs[1] if D == 2 else (None,) * 4
        hprev = torch.ops.ptmi.chunk_gru_backward(gates, q, dh.contiguous(), dirs[0][1], rev[1], h, table, cap, H, flip)
        need = ctx.needs_input_grad
        bias = dirs[0][2] is not None
        if bias:
            db_ih, db_hh = torch.ops.ptmi.dprnn_colsum_pair(gates)          # (dr_pre, dz_pre, dn_pre): b_ih, and b_hh's r and z blocks
            db_hh.view(D, 3, H)[:, 2] = torch.ops.ptmi.dprnn_colsum(q).view(D, H)      # b_hn sees dn_pre r
        grads, dx = [], None
        for d, (w_ih, _, _, _) in enumerate(dirs):
            dg = gates[:, d * 3 * H:(d + 1) * 3 * H]
            hp = hprev[:, d * H:(d + 1) * H]
            dw_hh = torch.empty((3 * H, H), dtype=torch.float32, device=x.device)
            _gemm.mm(dg[:, :2 * H].t(), hp, out=dw_hh[:2 * H])
            _gemm.mm(q[:, d * H:(d + 1) * H].t(), hp, out=dw_hh[2 * H:])
            grads += [_gemm.mm(dg.t(), x), dw_hh, db_ih[d * 3 * H:(d + 1) * 3 * H] if bias else None,
                      db_hh[d * 3 * H:(d + 1) * 3 * H] if bias else None]
            if need[0]:
                dx = _gemm.mm(dg, w_ih) if dx is None else _gemm.mm(dg, w_ih, out=dx, accumulate=True)
        grads += [None] * (len(params) - len(grads))
        return (dx, None, None, None, *[g if nd else None for g, nd in zip(grads, need[4:])])


def chunk_gru(x, table, cap, w_ih, w_hh, b_ih=None, b_hh=None, w_ih_reverse=None, w_hh_reverse=None, b_ih_reverse=None,
              b_hh_reverse=None, flip=False):
    """``x [rows, N]`` -> ``h [rows, D H]``: one GRU layer with the parameters of ``torch.nn.GRU`` (``weight_ih [3H, N]``, ``weight_hh
    [3H, H]``, ``bias_ih``, ``bias_hh [3H]`` or both None; gate order r, z, n; the ``_reverse`` four make it bidirectional) over the
    sequences of ``table [nseq, 3]`` int32 = (base row, step stride, step count <= cap); see the module's docstring for the contract."""
    params = [w_ih, w_hh, b_ih, b_hh, w_ih_reverse, w_hh_reverse, b_ih_reverse, b_hh_reverse]
    _check('chunk_gru', x, *params)
    if x.dim() != 2 or x.numel() == 0 or not x.is_contiguous():
        raise ValueError(f'chunk_gru: x [rows, N] contiguous, got {tuple(x.shape)} with strides {x.stride()}')
    if table.dtype != torch.int32 or table.dim() != 2 or table.shape[1] != 3 or table.shape[0] < 1 or not table.is_cuda:
        raise ValueError(f'chunk_gru: table [nseq, 3] int32 on the GPU, got {table.dtype} {tuple(table.shape)} on {table.device}')
    if int(cap) < 1:
        raise ValueError(f'chunk_gru: cap >= 1, got {cap}')
    if w_ih is None or w_hh is None or (w_ih_reverse is None) != (w_hh_reverse is None):
        raise ValueError('chunk_gru: weight_ih and weight_hh per direction')
    H, N = w_hh.shape[1], x.shape[1]
    dirs = _directions(params)
    for w_i, w_h, b_i, b_h in dirs:
        if tuple(w_i.shape) != (3 * H, N) or tuple(w_h.shape) != (3 * H, H):
            raise ValueError(f'chunk_gru: weight_ih [{3 * H}, {N}] and weight_hh [{3 * H}, {H}], got {tuple(w_i.shape)}, {tuple(w_h.shape)}')
        if (b_i is None) != (b_h is None) or (b_i is None) != (b_ih is None) or (b_i is not None and (b_i.shape != (3 * H,) or b_h.shape != (3 * H,))):
            raise ValueError(f'chunk_gru: bias_ih and bias_hh [{3 * H}] in every direction, or none at all')
    if H > MAX_HIDDEN:
        raise NotImplementedError(f'chunk_gru: hidden_size {H} > {MAX_HIDDEN}: the recurrence kernels keep the recurrent gate gradients, dh '
                                  f'and its carry of a tile of four sequences in LDS: 80 bytes per unit of the 160 KB of a CU')
    params = [None if p is None else p.contiguous() for p in params]
    return _ChunkGruFn.apply(x, table.contiguous(), int(cap), bool(flip), *params)
