"""Packed-sequence (B)LSTM on MI355X: drop-in compute path for ``torch.nn.LSTM(PackedSequence)``.

``packed_lstm(lstm, packed)`` evaluates a ``torch.nn.LSTM`` module (its own parameters - the
``state_dict`` layout of the reference models is untouched) on a
``PackedSequence`` exactly like ``lstm(packed)[0]`` as used at
``padertorch/contrib/examples/source_separation/pit/model.py:97`` and ``contrib/tcl/dc.py:61``:

* per layer ONE dense GEMM ``X [W_ih_fwd; W_ih_rev]^T + (b_ih + b_hh)`` for both directions (BLAS);
* the time recurrence runs in the HIP kernels of ``csrc/lstm.hip`` (``ptmi_lstm_forward`` /
  ``ptmi_lstm_backward``): one launch per timestep for both directions, exact fp32 on the matrix
  cores, fused gate non-linearities, activations saved in place for the backward pass;
* weight / input gradients are dense GEMMs on the saved gate gradients.

This module holds the layer function, ``packed_lstm`` and the process-default switches.  The batch tables are
``ops.pack_meta``, the parameter forms and their queues ``ops.lstm_forms``, the weight-gradient queue ``ops.wgrad``, the
persistent kernels' error word ``ops.watchdog``; their public names are re-exported here.
"""
import types

import torch
from torch.nn.utils.rnn import PackedSequence

from .. import _lib
from . import capture as _capture
from . import context as _context
from . import gemm as _gemm
from . import library  # noqa: F401  (registers torch.ops.ptmi.*)
from . import lstm_forms as _forms
from . import watchdog as _watchdog
from . import wgrad as _wgrad
from .lstm_forms import begin_captured_step, end_captured_step  # noqa: F401
from .pack_meta import _PackMeta, _meta, pack_meta  # noqa: F401
from .watchdog import check_errors, error_count, error_word, errors_since_last_report, raise_timeout  # noqa: F401
from .wgrad import flush_pending as flush_pending_wgrad, gemm_keys_safe, sync_deferred, warm_side_stream, wgrad_key  # noqa: F401

__all__ = ['packed_lstm']


#: run the forward recurrence as ONE persistent launch per layer (W_hh resident in registers)
PERSISTENT = True
#: read back the error words of the persistent kernels after every call (host sync; tests only)
CHECK_PERSISTENT_ERRORS = False
#: Accumulate the weight gradients of the LSTM layers straight into the parameters' ``.grad`` buffers
#: (set by the Trainer when it owns flat gradient buffers) - and do so on a SIDE stream where that is
#: safe: the backward recurrence of the next (lower) layer occupies ~150-200 of the 256 CUs exclusively
#: (its workgroups hold a CU's whole register file), so the dW GEMMs of the layer above run on the idle
#: CUs meanwhile (bench config: 18.2 -> 17.4 ms per step, C3: 64 -> 60).
#: HAZARD and its guard: the persistent recurrence kernels need all their workgroups co-resident.  A
#: kernel running next to them must never wait for its own not-yet-dispatched workgroups, or the two
#: starve each other: hipBLASLt's Stream-K GEMMs (``SK3`` in their names) do, and with them the first
#: unsynchronised step at B = 64, T = 503 hung the GPU every time.  rocBLAS' tiled kernels do not (split-K
#: goes through a second kernel), so the side stream is used ONLY for shapes whose TunableOp entry pins
#: a rocBLAS solution (``_side_stream_safe``; ``scripts/tune_gemms.py --overlap`` produces them; 15 cold
#: starts over five configurations ran clean); every other shape accumulates on the main stream.
#: ``sync_deferred()`` must run before anything reads the gradients (the Trainer does).
DEFER_WGRAD = False
#: called with the list of parameters whose gradients have just been accumulated in place (the data-parallel
#: Trainer issues the layer's all-reduce from it; autograd's post-accumulate hooks do not fire for in-place writes)
GRAD_READY_HOOK = None
#: called in the FORWARD pass with the parameters of a module whose weight gradients the backward pass will accumulate in place:
#: one call per use, so that a module applied twice is reported ready only after its last backward use (GradBuckets.expect)
GRAD_USE_HOOK = None
#: False: the deferred accumulation runs on the current stream (same GEMM shapes, no overlap; used by the
#: one-off GEMM tuning, which must not time kernels next to a running recurrence)
WGRAD_SIDE_STREAM = True
#: LSTM input gradients on the planes GEMM straight from the backward recurrence's hand-off planes (no pack pass)
DX_FROM_HANDOFF = True
#: the top layer's backward recurrence runs in two launches for batches of at least this many packed rows (see _backward_plan)
SPLIT_TOP_BACKWARD_ROWS = 16384


# (Always on since they were measured - rounds 2-4, DESIGN.md sections 3.3 / 3.9 / 4 - and no switches any more: per-version cached stacked
#  weights; the first layer's weight gradients on both queues (the step's tail); the backward scratch's data-as-flag pattern written by the
#  forward recurrence kernel; the forward recurrence's hand-off planes as operand A of the next projection / dense layer; the gate gradients
#  handed to the weight-gradient GEMMs as bf16 planes of dgates^T by the backward kernel; both directions' dW_ih as one launch.)
#: attribute of a packed_lstm output tensor whose recurrence has left it as hand-off planes: (version, (scratch, cols), ndir, H)
HANDOFF_ATTR = '_ptmi_handoff_planes'


def handoff_planes_of(x):
    """``((scratch, cols), ndir, H)`` when ``x`` is an output tensor of :func:`packed_lstm` that still holds what its recurrence
    wrote (same object, no in-place edit since), else ``None``."""
    rec = getattr(x, HANDOFF_ATTR, None)
    if rec is None or rec[0] != x._version:
        return None
    return rec[1:]


def _side_stream_safe(rows, I, H, ndir, shifted_views):
    """`shifted_views`: h_{t-1} is a column block of the padded output buffer (row stride ndir * H), not a
    gathered copy."""
    G = 4 * H
    return gemm_keys_safe((wgrad_key(I, G, rows, ndir * G),
                           wgrad_key(H, G, rows, ndir * G, ndir * H if shifted_views else None)))


def _input_projection(x, w_ih, bias, meta, ndir, G, H, forms, prev, params, x_unit):
    """``gates = x W_ih^T + bias`` ``[rows, ndir 4H]`` on the best operand form at hand.  Returns ``(gates, x, gm)``: ``x`` as the
    backward pass is to multiply it (a view with a padded row stride when the reduction axis was padded), ``gm`` the operand
    scales ``(amax_x, amax_w)`` of the split GEMM or ``None`` (library GEMM)."""
    use_gemm = _gemm.usable(x, w_ih)
    planes_ok = use_gemm and _gemm.planes_enabled() and forms is not None
    # operand ranges of the split GEMM: the layer input is taken as it is when it is a hidden state (|h| < 1,
    # a dropout scale aside), measured otherwise; the stacked weights' maximum is cached per optimizer step
    hplanes = prev.get('planes') if prev else None
    xplanes = prev.get('xplanes') if prev else None
    if not (xplanes is not None and planes_ok and forms.w_ih_planes is not None):
        xplanes = None
    if not use_gemm:
        return torch.addmm(bias, x, w_ih.t()), x, None
    amax_x = (_gemm.UNIT_RANGE if x_unit else _gemm.scale_word(x.device, xplanes[1]) if xplanes is not None else _gemm.absmax(x))
    amax_w = _gemm.weights_absmax([ps[0] for ps in params]) if params is not None else _gemm.absmax(w_ih)
    if xplanes is not None:
        # the producer of x has left it as fp16 planes with a fixed operand scale (the feature kernel: 2^9 log1p|Y|);
        # the same scale word serves the weight gradient's pack of the fp32 x in the backward pass
        gates = torch.empty((meta.rows, ndir * G), dtype=torch.float32, device=x.device)
        wpl = forms.input_planes()
        torch.ops.ptmi.gemm_planes_(gates, xplanes[0], amax_x, wpl[0], wpl[1], bias, meta.rows, ndir * G, x.shape[1], False, 1)
    elif hplanes is not None and planes_ok and forms.w_ih_planes_h is not None and forms.w_ih_planes_h[1] == hplanes[1]:
        # the previous layer's recurrence has left its output as fp16 (hi, lo) planes of 2^10 h in fragment order (its
        # hand-off copy): operand A of this projection as it lies, no pack pass
        gates = torch.empty((meta.rows, ndir * G), dtype=torch.float32, device=x.device)
        kh = (x.shape[1] // H) * hplanes[1]
        wpl = forms.w_ih_planes_h[0]
        torch.ops.ptmi.gemm_planes_(gates, hplanes[0], _gemm.scale_word(x.device), wpl[0], wpl[1], bias, meta.rows, ndir * G, kh,
                                    False, _gemm.auto_split_k(meta.rows, ndir * G, kh))
    elif planes_ok and forms.w_ih_planes is not None:
        # both operands as fp16 planes: the input split once here, the stacked weights' planes come with the forms
        gates = torch.empty((meta.rows, ndir * G), dtype=torch.float32, device=x.device)
        _gemm.mm_planes_(gates, _gemm.pack_n(x, amax_x), forms.input_planes(), meta.rows, ndir * G, x.shape[1], bias=bias)
    else:
        # an input width that is not a multiple of 4 (F = 257) would send the projection and its weight gradient
        # down the kernel's unaligned (scalar-load) path: zero-pad the reduction axis of both operands instead
        kpad = -x.shape[1] % 4
        if kpad:
            x_in = x
            x = torch.nn.functional.pad(x_in, (0, kpad))
            w_ih_k = forms.w_ih_kpad if forms is not None else torch.nn.functional.pad(w_ih, (0, kpad))
            gates = _gemm.mm(x, w_ih_k.t(), bias=bias, amax_x=amax_x, amax_y=amax_w)
            x = x[:, :x_in.shape[1]]                  # view with the padded row stride: what the backward pass multiplies
        else:
            gates = _gemm.mm(x, w_ih.t(), bias=bias, amax_x=amax_x, amax_y=amax_w)
    return gates, x, (amax_x, amax_w)


def _backward_plan(ctx, lib, x, h0, ndir, H, has_grads, has_dc):
    """What the backward pass of one layer will do, decided once (nothing is enqueued here; the side stream is looked up).

    ``in_place``: weight gradients accumulated into ``.grad`` (see DEFER_WGRAD), on ``side`` - the side stream where that is safe
    (``use_side``): the split GEMM kernels never wait for sibling workgroups - always safe next to a persistent recurrence -,
    library kernels only when their shape is pinned to a rocBLAS solution -, else ``main``.
    ``state_grad``: gradients w.r.t. the initial state (the range entry point leaves the cell-state gradient behind the last step)
    or from the final cell state (``has_dc``: the states entry point of the range launcher).
    ``chunks``: launches of the recurrence.  The TOP layer's backward recurrence runs while the weight-gradient queue is still
    empty; for long batches, where that queue is the critical one of the backward phase (16 kHz configurations: 11.9 ms of GEMMs
    and pack passes beside 9.7 ms of recurrences), it runs as two launches over step ranges and the finished half's weight
    gradients start under the second launch (s_begin / s_end of ptmi_lstm_backward_persistent).  For every layer, or at B = 32 / T = 253, the
    same cut measured neutral to slower (a recurrence next to GEMMs loses what the GEMMs gain): c3 23.97 -> 23.55 ms with the top
    layer in two launches, 23.35 / 23.33 in three / four, 23.70 with every layer in two.
    (The BOTTOM layer in two launches - its first half's weight gradients under its second launch instead of in the step's tail -
    measured in the captured step, round 5: c2 6.60 -> 6.90 ms, c3 21.4 -> 22.0, c5 18.1 -> 18.5.  The replay's timeline: the side
    queue has no room in that window - the layer above's weight gradients (0.45 ms) run there, and as captured they ended up BEHIND
    the first range's -, two launches take 36 us longer than one, and the last range's GEMMs lose the two-queue tail.)
    ``use_tp``: the gate gradients come as bf16 planes of dgates^T straight from the kernel (no row-major fp32 tensor at all when
    the input gradient takes the hand-off planes - ``cols_dx`` columns per direction, ``uniform_rows`` -, or is not needed)."""
    meta, gm, oc = ctx.meta, ctx.gemm, ctx.oc
    p = types.SimpleNamespace()
    p.in_place = (oc.defer_wgrad or ctx.forms is not None) and has_grads
    p.use_side = p.in_place and oc.wgrad_side_stream and (
        gm is not None or _side_stream_safe(meta.rows, x.shape[1], H, ndir, ctx.ext is not None))
    p.main = torch.cuda.current_stream(x.device) if p.in_place else None
    p.side = _wgrad.stream(x.device) if p.use_side else p.main
    p.state_grad = h0 is not None and (any(ctx.needs_input_grad[5:7]) or has_dc)
    p.masks = meta.masks_dev                 # row-slot batch
    p.chunks = 2 if (ctx.top and PERSISTENT and p.use_side and gm is not None
                     and _gemm.planes_enabled() and lib.ptmi_lstm_split_enabled() and meta.T >= 128
                     and meta.rows >= SPLIT_TOP_BACKWARD_ROWS and p.masks is None) else 1
    p.cols_dx = int(lib.ptmi_lstm_handoff_cols(H, 1)) if DX_FROM_HANDOFF else 0
    p.uniform_rows = meta.uniform_rows
    dx_needs_rows = ctx.needs_input_grad[0] and not (p.cols_dx and p.uniform_rows)
    p.use_tp = bool(PERSISTENT and p.in_place and gm is not None and _gemm.planes_enabled()
                    and not p.state_grad and not dx_needs_rows
                    and lib.ptmi_lstm_backward_planes_ok(meta.T, ndir, meta.max_batch, meta.rows, H))
    return p


def _backward_scratch(lib, meta, scratch_b, pre_b, ndir, H, device):
    """``(scratch, prefilled)`` of a backward launch: the one the forward recurrence has prefilled, or a fresh one the launch fills."""
    if scratch_b is not None:
        return scratch_b, int(pre_b)
    return torch.empty(int(lib.ptmi_lstm_scratch_elems(meta.T, ndir, meta.max_batch, H, 1)), dtype=torch.int32, device=device), 0


def _scratch_tail(lib, flags, meta, ndir, G):
    """Views into the tail of a backward scratch, ``[bias gradient [ndir * 4H] | 8 words, word 0 = max |dgates| | slots | error
    words]``: ``(bias sums as fp32, maximum word)``."""
    end = flags.numel() - (int(lib.ptmi_lstm_flags_elems(meta.T, ndir, meta.max_batch)) + 8)
    return flags[end - ndir * G:end].view(torch.float32), flags[end:end + 1]


def _launch_planes_range(lib, meta, saved, flags, carry, pre, masks, ndir, G, H, t0, t1):
    """One launch of the planes recurrence over the steps ``t0 .. t1``: ``(ok, planes of dgates^T, row ranges per direction)``."""
    gates, c, c0, dhy, w_t = saved
    T, B_ = meta.T, meta.max_batch
    planes = torch.empty(ndir * int(lib.ptmi_planes_elems(G, (t1 - t0) * B_)), dtype=torch.bfloat16, device=dhy.device)
    ok = torch.ops.ptmi.lstm_recurrence_backward_planes(
        gates, c, c0, dhy, w_t, None, planes, flags, carry, meta.bs_dev, meta.offs_dev, T, B_, meta.rows, H, ndir, t0, t1, pre, masks)
    # rows of this range per direction (forward direction: processed from the last time index down)
    return ok, planes, [((T - t1) * B_, (T - t0) * B_), (t0 * B_, t1 * B_)][:ndir]


def _backward_planes(lib, meta, plan, job, saved, scratch_b, pre_b, ndir, G, H):
    """The recurrence that leaves bf16 planes of dgates^T, in ``plan.chunks`` launches; a finished range's weight gradients start
    under the next launch.  ``(dg, dg_t, flags, carry, todo)`` - ``todo``: the row ranges whose weight gradients are still to be
    accumulated -, or ``None`` when the launch was refused (another path decides)."""
    device, chunks, T = saved[3].device, plan.chunks, meta.T
    flags, pre = _backward_scratch(lib, meta, scratch_b, pre_b, ndir, H, device)
    cuts = [T * i // chunks for i in range(chunks + 1)]
    carry = torch.empty((ndir, meta.max_batch, H), dtype=torch.float32, device=device) if chunks > 1 else None
    ok, dg_t, part_t = _launch_planes_range(lib, meta, saved, flags, carry, pre, plan.masks, ndir, G, H, cuts[0], cuts[1])
    if not ok:
        return None
    for i in range(1, chunks):
        done = torch.cuda.Event()
        done.record(plan.main)
        finished, finished_part = dg_t, part_t
        # (the next range's launch is enqueued FIRST: a captured step is laid out in capture order, and the recurrence must
        #  not end up behind the side queue's GEMMs - ops.wgrad)
        ok, dg_t, part_t = _launch_planes_range(lib, meta, saved, flags, carry, pre, plan.masks, ndir, G, H, cuts[i], cuts[i + 1])
        if not ok:
            raise RuntimeError('ptmi_lstm_backward_persistent: a later range was refused')
        plan.side.wait_event(done)
        job.rows(None, finished_part, None, dg_t=finished)        # the finished range, under the next launch
        finished.record_stream(plan.side)
    return None, dg_t, flags, carry, part_t


def _backward_ranges(lib, meta, plan, job, saved, scratch_b, pre_b, ndir, G, H, dcn):
    """The fp32 recurrence over step ranges (several launches, or gradients w.r.t. the states: ``carry`` is the cell-state
    gradient behind the last step).  Same result tuple as :func:`_backward_planes`."""
    gates, c, c0, dhy, w_t = saved
    chunks, T = plan.chunks, meta.T
    dg = torch.empty_like(gates)
    flags, pre = _backward_scratch(lib, meta, scratch_b, pre_b, ndir, H, dhy.device)
    carry = torch.empty((ndir, meta.max_batch, H), dtype=torch.float32, device=dhy.device)
    cuts = [T * i // chunks for i in range(chunks + 1)]
    amax_word = _scratch_tail(lib, flags, meta, ndir, G)[1]
    offs = [int(v) for v in meta.offs_host[:T]] + [meta.rows]
    todo = [(0, meta.rows)] * ndir
    for i in range(chunks):
        if i:
            snap = amax_word.clone()                     # max |dgates| so far: the operand scale of this part
            done = torch.cuda.Event()
            done.record(plan.main)
            plan.side.wait_event(done)
            s0, s1 = cuts[i - 1], cuts[i]                # steps finished by the previous launch
            job.rows(dg, [(offs[T - s1], offs[T - s0]), (offs[s0], offs[s1])][:ndir], snap)
            snap.record_stream(plan.side)
        ok = torch.ops.ptmi.lstm_recurrence_backward_range(
            gates, c, c0, dhy, w_t, dg, flags, carry, meta.bs_dev, meta.offs_dev, T, meta.max_batch, meta.rows, H,
            ndir, cuts[i], cuts[i + 1], pre, dcn)
        if not ok:
            if i:
                raise RuntimeError('ptmi_lstm_backward_persistent: a later range was refused')
            if plan.state_grad:                          # (else not resident: the one-call path decides)
                raise NotImplementedError('gradients w.r.t. the initial LSTM state: this configuration cannot run on the '
                                          'persistent kernels')
            return None
    if chunks > 1:
        s0 = cuts[chunks - 1]
        todo = [(offs[0], offs[T - s0]), (offs[s0], offs[T])][:ndir]
    return dg, None, flags, carry, todo


def _backward_one_call(meta, plan, saved, scratch_b, pre_b, ndir, H):
    """The whole recurrence in one call of the op (persistent when it fits, else a launch per step).  Same result tuple."""
    gates, c, c0, dhy, w_t = saved
    dg, flags = torch.ops.ptmi.lstm_recurrence_backward(
        gates, c, c0, dhy, w_t, meta.bs_dev, meta.offs_dev, meta.bs_host.ctypes.data, meta.offs_host.ctypes.data,
        meta.T, meta.max_batch, meta.rows, H, ndir, PERSISTENT, scratch_b, int(pre_b), plan.masks)
    return dg, None, flags, None, [(0, meta.rows)] * ndir


def _input_grad(ctx, lib, plan, dg, flags, amax_dg, amax_kernel, w_ih, ndir, H):
    """``dx = dgates W_ih`` ``[rows, I]`` (``None`` when the layer input needs none)."""
    meta, gm, params = ctx.meta, ctx.gemm, ctx.params
    if not ctx.needs_input_grad[0]:
        return None
    if gm is None:
        return dg @ w_ih
    cols = plan.cols_dx if (flags is not None and amax_kernel is not None) else 0
    if cols and _gemm.planes_enabled() and plan.uniform_rows:
        # the recurrence has left its gate gradients as bf16 (hi, lo) planes in fragment order at the start of its
        # scratch (the hand-off copy): for a batch of equal lengths they ARE operand A of dx = dgates W_ih
        pdx = ctx.forms.w_ih_planes_dx if ctx.forms is not None else None
        wplanes = pdx[0] if (pdx is not None and pdx[1] == cols) else _gemm.stacked_planes_t_bf16(
            w_ih, ndir, cols, None if params is None else [ps[0] for ps in params])
        dx = torch.empty((meta.rows, w_ih.shape[1]), dtype=torch.float32, device=flags.device)
        torch.ops.ptmi.gemm_planes_bf16_(dx, flags, 0, wplanes, None, meta.rows, w_ih.shape[1], ndir * cols, False,
                                         _gemm.auto_split_k(meta.rows, w_ih.shape[1], ndir * cols))
        return dx
    return _gemm.mm(dg, w_ih, amax_x=amax_dg, amax_y=gm[1])


#: a BLSTM layer's four weight gradients (both directions' dW_ih and dW_hh) over the recurrence's bf16 planes of dgates^T as ONE pack
#: launch (x, h_prev forward, h_prev reverse) and ONE grouped GEMM launch with one slab reduction (``ptmi_gemm_planes_bf16_group``)
#: instead of the fused dW_ih call and the two dW_hh calls with a pack and a reduction each.  Off: exactly those calls (tests, A/B runs).
GROUP_WGRAD = True


class _WgradJob:
    """The in-place weight gradients of one layer's backward pass: :meth:`rows` accumulates dW_ih / dW_hh over row ranges (as
    often as the recurrence is cut), :meth:`accumulate` the rest and the biases - at once or parked on ``ops.wgrad``.  Owns what
    the calls share: ``operands`` (per direction: gate gradients, h_{t-1}), ``xplanes`` / ``dgplanes`` (packed operands per row
    range)."""

    def __init__(self, ctx, lib, plan, x, hy, h0, ndir, H):
        self.lib, self.plan, self.meta, self.gm, self.params, self.oc = lib, plan, ctx.meta, ctx.gemm, ctx.params, ctx.oc
        self.x, self.hy, self.h0, self.ext, self.ndir, self.H, self.G = x, hy, h0, ctx.ext, ndir, H, 4 * H
        self.first_layer = not ctx.needs_input_grad[0]
        self.operands, self.xplanes, self.dgplanes, self.group = None, {}, {}, {}

    def rows(self, dg, ranges, amax_dg, both_queues=False, dg_t=None):
        """dW_ih, dW_hh of every direction d over the rows ranges[d] = (r0, r1) of the packed batch, on `side`
        (both_queues: all but the forward direction's dW_hh on the main stream - the step's tail, see `share_operands`).
        dg_t: the kernel's bf16 planes of dgates^T for exactly these row ranges (then `dg` is None); with both directions over ONE row
        range all four products go out as one grouped call (`GROUP_WGRAD`) on one queue: `main` for both_queues, else `side`."""
        lib, gm, params, x, h0, ndir, H, G = self.lib, self.gm, self.params, self.x, self.h0, self.ndir, self.H, self.G
        main, side, xplanes = self.plan.main, self.plan.side, self.xplanes
        if self._grouped(dg_t, ranges):
            # all four products reduce over the same packed rows and share operands (x: both dW_ih; each direction's dgates^T: its
            # dW_ih and dW_hh): one pack launch, one GEMM launch over the tiles of all four, one slab reduction
            r0, r1 = ranges[0]
            with torch.cuda.stream(main if both_queues else side):
                if self.operands is None:
                    self.operands = _recurrent_operands(self.meta, dg, self.hy, self.ext, h0, ndir, H)
                px, pf, pb = torch.ops.ptmi.pack_planes_bf16_list([x[r0:r1], self.operands[0][1][r0:r1], self.operands[1][1][r0:r1]])
                ok = torch.ops.ptmi.gemm_planes_bf16_group_(
                    [params[0][0].grad, params[0][1].grad, params[1][0].grad, params[1][1].grad], self.GROUP_BLOCKS, dg_t, 0, 2 * G, G,
                    [px, pf, pb], [x.shape[1], H, H], r1 - r0, True, _gemm.auto_split_k(G, H, r1 - r0))
                assert ok, 'ptmi_gemm_planes_bf16_group refused a call its plan had accepted'
            return
        # both directions' dW_ih = [dgates_f | dgates_r]^T x share the operand x and the kernel's planes of dgates^T lie behind each
        # other: ONE launch with a two-part output (ptmi_gemm_planes_bf16_two) instead of two GEMMs + two slab reductions
        fused_ih = False
        if (dg_t is not None and ndir == 2 and ranges[0] == ranges[1] and ranges[0][1] > ranges[0][0]):
            ga, gb = params[0][0].grad, params[1][0].grad
            if ga.stride() == gb.stride() and (ga.data_ptr() ^ gb.data_ptr()) & 15 == 0 and ga.is_contiguous():
                r0, r1 = ranges[0]
                with torch.cuda.stream(main if both_queues else side):
                    key = (r0, r1)
                    if key not in xplanes:
                        xplanes[key] = torch.ops.ptmi.pack_planes_bf16(x[r0:r1], True)
                    torch.ops.ptmi.gemm_planes_bf16_two_(ga, gb, dg_t, 0, xplanes[key], 2 * G, x.shape[1], r1 - r0, True,
                                                         _gemm.auto_split_k(2 * G, x.shape[1], r1 - r0))
                fused_ih = True
        for d, ((p_wih, p_whh, _, _), (r0, r1)) in enumerate(zip(params, ranges)):
            q_ih = main if both_queues else side
            q_hh = main if both_queues and d == 1 else side
            with torch.cuda.stream(q_ih):
                if self.operands is None:
                    self.operands = _recurrent_operands(self.meta, dg, self.hy, self.ext, h0, ndir, H)
                dgd, h_prev = self.operands[d]
                if r1 <= r0:
                    continue
                if dg_t is not None:
                    # both operands reduce over the packed rows: dgates^T comes from the recurrence as bf16 planes; the layer
                    # input (once for both directions) and the previous hidden state are packed to match (bf16: no scale)
                    k = r1 - r0
                    key = (r0, r1)
                    a_off = d * int(lib.ptmi_planes_elems(G, k)) * 2
                    if key not in xplanes and not fused_ih:
                        xplanes[key] = torch.ops.ptmi.pack_planes_bf16(x[r0:r1], True)
                    if not fused_ih:
                        torch.ops.ptmi.gemm_planes_bf16_(p_wih.grad, dg_t, a_off, xplanes[key], None, G, x.shape[1], k, True,
                                                         _gemm.auto_split_k(G, x.shape[1], k))
                    with torch.cuda.stream(q_hh):
                        hpl = torch.ops.ptmi.pack_planes_bf16(h_prev[r0:r1], True)
                        torch.ops.ptmi.gemm_planes_bf16_(p_whh.grad, dg_t, a_off, hpl, None, G, H, k, True, _gemm.auto_split_k(G, H, k))
                    continue
                dgt = dgd[r0:r1].t()
                if gm is not None and _gemm.planes_enabled():
                    # both operands reduce over the batch's rows (their outer axis): split them into fp16 planes once
                    # (dg for two GEMMs, the layer input for both directions) and run the plain 16-bit GEMM
                    k = r1 - r0
                    key = (r0, r1)
                    dgp = self.dgplanes.get((d, key))
                    if dgp is None:
                        dgp = _gemm.pack_t(dgd[r0:r1], amax_dg)
                    if key not in xplanes:
                        xplanes[key] = _gemm.pack_t(x[r0:r1], gm[0])
                    _gemm.mm_planes_(p_wih.grad, dgp, xplanes[key], G, x.shape[1], k, accumulate=True, split_k=_gemm.auto_split_k(G, x.shape[1], k))
                    with torch.cuda.stream(q_hh):
                        hpl = _gemm.pack_t(h_prev[r0:r1], _gemm.UNIT_RANGE if h0 is None else None)
                        _gemm.mm_planes_(p_whh.grad, dgp, hpl, G, H, k, accumulate=True, split_k=_gemm.auto_split_k(G, H, k))
                elif gm is not None:
                    _gemm.mm(dgt, x[r0:r1], out=p_wih.grad, accumulate=True, amax_x=amax_dg, amax_y=gm[0])
                    _gemm.mm(dgt, h_prev[r0:r1], out=p_whh.grad, accumulate=True, amax_x=amax_dg,
                             amax_y=_gemm.UNIT_RANGE if h0 is None else None)
                else:
                    p_wih.grad.addmm_(dgt, x[r0:r1])
                    p_whh.grad.addmm_(dgt, h_prev[r0:r1])

    #: blocks (part * 3 + segment) of the grouped call: (dG_f, x), (dG_f, h_f), (dG_b, x), (dG_b, h_b)
    GROUP_BLOCKS = [0, 1, 3, 5]

    def _grouped(self, dg_t, ranges):
        """Whether :meth:`rows` takes the grouped call for these ranges: the recurrence's planes of both directions over one row range,
        and a shape the big-tile kernel runs (else: the separate calls).  Decided once per row range."""
        if not (GROUP_WGRAD and dg_t is not None and self.ndir == 2 and ranges[0] == ranges[1] and ranges[0][1] > ranges[0][0]):
            return False
        key = ranges[0]
        if key not in self.group:
            grads = [ps[i].grad for ps in self.params for i in (0, 1)]
            k = key[1] - key[0]
            self.group[key] = all(g is not None and g.dim() == 2 and g.stride(1) == 1 and g.dtype == torch.float32 for g in grads) and \
                _gemm.group_plan(2 * self.G, self.G, [self.x.shape[1], self.H, self.H], self.GROUP_BLOCKS, k,
                                 _gemm.auto_split_k(self.G, self.H, k)) // 100 != 5
        return self.group[key]

    def finish(self, dg, dg_t, todo, amax_dg, db_kernel):
        """The rest of the layer's weight gradients (rows ``todo``) and its bias gradients, enqueued here or - a captured step -
        behind the next lower layer's recurrence launch."""
        plan, params, x, ndir, gm = self.plan, self.params, self.x, self.ndir, self.gm
        self.dg, self.dg_t, self.todo, self.amax_dg, self.db_kernel = dg, dg_t, todo, amax_dg, db_kernel
        # the first layer's weight gradients are the step's tail (nothing but the optimizer follows), and the side queue reaches
        # them ~0.25 ms after the main queue has gone idle (it still has the layer above's GEMMs: scripts/phase_events.py): all
        # but the forward direction's dW_hh go to the main queue, so that the side queue is done first and the optimizer does
        # not start behind a cross-queue hand-over (small launches with ~12 us of dispatch gap between dependent kernels of
        # one queue; a wait for an event that has not fired yet costs 30-60 us)
        self.both = both = (plan.use_side and ndir > 1 and gm is not None and _gemm.planes_enabled()
                            and self.first_layer and todo[0] == (0, self.meta.rows))
        if both:
            # (one grouped launch: all of it on the main queue - nothing to share between the queues)
            group = self._grouped(dg_t, todo)
            # earlier side-stream accumulations into the same .grad views
            _wgrad.wait_done(plan.main, (params[0][0], params[1][0], params[1][1]) + ((params[0][1],) if group else ()))
            self.operands = _recurrent_operands(self.meta, dg, self.hy, self.ext, self.h0, ndir, self.H)
            # shared between the queues: packed before they part
            if dg_t is not None and not group:
                self.xplanes[todo[0]] = torch.ops.ptmi.pack_planes_bf16(x, True)
            elif dg_t is None:
                self.xplanes[todo[0]] = _gemm.pack_t(x, gm[0])
                self.dgplanes[(0, todo[0])] = _gemm.pack_t(self.operands[0][0], amax_dg)
        # captured steps: enqueue behind the next lower layer's recurrence launch (ops.wgrad.defer); the side stream waits for the
        # event of THIS point, as it would have
        self.here = None
        if _capture.ACTIVE and plan.use_side and not both and not self.first_layer:
            self.here = torch.cuda.Event()
            self.here.record(plan.main)
            _wgrad.defer(self.accumulate)
        else:
            self.accumulate()

    def accumulate(self, _start=None):
        plan, params, x, oc = self.plan, self.params, self.x, self.oc
        main, side, use_side, both = plan.main, plan.side, plan.use_side, self.both
        dg, dg_t, todo, amax_dg, db_kernel = self.dg, self.dg_t, self.todo, self.amax_dg, self.db_kernel
        if use_side:
            if self.here is not None:
                side.wait_event(self.here)
            else:
                side.wait_stream(main)
        else:
            main.wait_stream(_wgrad.stream(x.device))      # earlier accumulations into the same .grad views
        self.rows(dg, todo, amax_dg, both_queues=both, dg_t=dg_t)
        with torch.cuda.stream(side):
            if db_kernel is not None and all(ps[2].grad.is_contiguous() and ps[3].grad.is_contiguous() for ps in params):
                # the kernel's bias sums into all 2 ndir bias gradients: one launch (was one small `add_` per bias vector)
                torch.ops.ptmi.lstm_bias_grad_add_(db_kernel, [ps[2].grad for ps in params], [ps[3].grad for ps in params])
            else:
                for d, (_, _, p_bih, p_bhh) in enumerate(params):
                    db_d = self.operands[d][0].sum(0) if db_kernel is None else db_kernel[d * self.G:(d + 1) * self.G]
                    p_bih.grad.add_(db_d)
                    p_bhh.grad.add_(db_d)
        done = None
        if use_side:
            done = torch.cuda.Event()
            done.record(side)
            _wgrad.mark_done([p for ps in params for p in ps[:2]], done)
        if both:
            main.wait_event(done)                          # the main queue is now behind both
            shared = self.dgplanes[(0, todo[0])][0] if dg_t is None else self.xplanes.get(todo[0])       # (grouped call: none)
            if shared is not None:
                shared.record_stream(side)
            if oc.grad_ready_hook is not None:
                side.wait_stream(main)                     # whoever orders itself after `side` sees every gradient
        if use_side:
            for t in (x, self.hy) + tuple(v for v in (dg, dg_t, self.h0, self.ext, db_kernel, amax_dg) if v is not None and torch.is_tensor(v)) \
                    + tuple(h_prev for _, h_prev in self.operands):
                t.record_stream(side)           # keep the operands alive until the side stream is done
        if oc.grad_ready_hook is not None:
            oc.grad_ready_hook([p for ps in params for p in ps])


class _LstmLayerFn(torch.autograd.Function):
    """x [rows, I] -> hy [rows, ndir*H] for one layer (both directions)."""

    @staticmethod
    def forward(ctx, x, w_ih, bias, w_hh, meta, h0=None, c0=None, params=None, x_unit=False, anchor=None, forms=None, prev=None,
                handoff=None, top=False, oc=None):
        # oc: ops.context.Effective of the LSTM module this layer belongs to (None: the process defaults)
        # prev: {'planes': (scratch, cols)} of the layer whose output `x` is (its hand-off planes as this projection's operand);
        # handoff: dict this call leaves its own planes in
        # anchor: a Parameter of the layer when (w_ih, bias, w_hh) are the cached detached forms (`forms`), so that the
        # node stays in the graph although none of its tensor inputs may require a gradient (first layer)
        lib = _lib.load()
        ndir, G, H = w_hh.shape
        assert G == 4 * H
        KP = _forms.kpad_of(H)
        ctx.set_materialize_grads(False)         # an unused output (the cell states of a call whose c_n nobody differentiates) comes back as None
        stateful = h0 is not None or c0 is not None
        if stateful:            # [ndir, B, H]; their gradients: see backward (persistent split kernels)
            h0 = torch.zeros_like(c0) if h0 is None else h0.detach().to(torch.float32).contiguous()
            c0 = torch.zeros_like(h0) if c0 is None else c0.detach().to(torch.float32).contiguous()
            assert h0.shape == c0.shape == (ndir, meta.max_batch, H), (h0.shape, c0.shape, meta.max_batch)
        # hand-off scratch of this layer's backward pass when one will come: the forward recurrence itself writes its data-as-flag
        # pattern into the planes (an idle wavefront per workgroup, a slice per time step); the forward scratch is allocated and
        # filled by the op
        scratch_b, pre_b = None, 0
        fills = int(lib.ptmi_lstm_forward_fills(meta.T, ndir, meta.max_batch, H)) if (
            PERSISTENT and x.is_cuda and any(ctx.needs_input_grad)) else 0
        if fills:
            scratch_b = torch.empty(int(lib.ptmi_lstm_scratch_elems(meta.T, ndir, meta.max_batch, H, 1)), dtype=torch.int32,
                                    device=x.device)
            pre_b = fills        # (2: the planes' pattern and the zeroed words behind them - the value the backward call takes as `prefilled`)
        gates, x, ctx.gemm = _input_projection(x, w_ih, bias, meta, ndir, G, H, forms, prev, params, x_unit)
        if stateful:        # h0 W_hh^T enters the pre-activations of each sequence's first processed step
            gv = gates.view(meta.rows, ndir, G)
            for d in range(ndir):
                gv[:, d].index_add_(0, meta.first_rows[d], h0[d] @ w_hh[d].t())
        if forms is not None:
            w_pad = forms.w_pad
        else:
            w_pad = torch.nn.functional.pad(w_hh, (0, KP - H)).contiguous() if KP != H else w_hh.contiguous()
        # equal-length batch: bs[0] rows of "state before the first step" (zero or h0) in front of and
        # behind the output rows, so that the backward pass reads h_{t-1} as a shifted view (no gather)
        pad = meta.bs0 if meta.equal_lengths else 0
        masks = meta.masks_dev          # row-slot batch (ops.sequence.SlotLayout): idle rows stay zero
        assert masks is None or not stateful, 'row-slot batches take no initial states'
        ext = (torch.zeros if masks is not None else torch.empty)((meta.rows + 2 * pad, ndir * H), dtype=torch.float32, device=x.device)
        hy = ext[pad:pad + meta.rows]
        if pad:
            # (both ends in ONE fill launch: a [2, pad, C] view over the first and the last `pad` rows)
            C_ = ndir * H
            torch.as_strided(ext, (2, pad, C_), ((pad + meta.rows) * C_, C_, 1)).zero_()
            if stateful:
                ext[:pad].view(pad, ndir, H)[:, 0] = h0[0]
                if ndir > 1:
                    ext[pad + meta.rows:].view(pad, ndir, H)[:, 1] = h0[1]
        ctx.ext = ext if pad else None
        # split-precision recurrence: the scale of W_hh's fp16 halves comes from its maximum (cached per optimizer step)
        amax_whh = None
        if PERSISTENT and lib.ptmi_lstm_split_enabled():
            amax_whh = (_gemm.weights_absmax([ps[1] for ps in params]) if params is not None
                        else _gemm.absmax(w_pad.view(-1, KP)))
        if PERSISTENT:
            _watchdog.arm(x.device)
        c, flags = torch.ops.ptmi.lstm_recurrence_forward(
            gates, hy, c0, w_pad, amax_whh, meta.bs_dev, meta.offs_dev, meta.bs_host.ctypes.data, meta.offs_host.ctypes.data,
            meta.T, meta.max_batch, meta.rows, H, KP, ndir, PERSISTENT, None, False, scratch_b, masks)
        if flags is None:        # the persistent launch was refused: nothing was filled
            pre_b = 0
        if handoff is not None and flags is not None and not stateful and meta.uniform_rows:
            cols_out = int(lib.ptmi_lstm_handoff_cols(H, 0))
            if cols_out:
                handoff['planes'] = (flags, cols_out)
        ctx.scratch_b = (scratch_b, pre_b)
        if flags is not None and CHECK_PERSISTENT_ERRORS:
            check_errors()
        ctx.save_for_backward(x, w_ih, w_hh, gates, c, hy, h0, c0)
        ctx.meta = meta
        ctx.params = params
        ctx.forms = forms
        ctx.top = bool(top)          # the layer whose backward pass runs first (nothing else is on the weight-gradient queue then)
        ctx.oc = oc if oc is not None else _context.effective(None)
        if stateful:
            return hy, c            # (c: differentiable too - the gradient of the FINAL cell state comes back through it, see backward)
        return hy

    @staticmethod
    def backward(ctx, dhy, _dc=None):
        meta = ctx.meta
        if dhy is None:             # only the cell states were used
            dhy = torch.zeros((meta.rows, ctx.saved_tensors[2].shape[0] * ctx.saved_tensors[2].shape[2]), dtype=torch.float32,
                              device=ctx.saved_tensors[0].device)
        lib = _lib.load()
        x, w_ih, w_hh, gates, c, hy, h0, c0 = ctx.saved_tensors
        # the backward scratch the forward recurrence has prefilled (pattern, zeroed bias sums / arrival words / error words) serves ONE
        # backward pass: this one leaves its hand-off planes and bias sums in it.  A second pass through the same graph
        # (retain_graph=True, torch.autograd.grad twice) takes a scratch of its own that its launch fills and zeroes (prefilled = 0)
        scratch_b, pre_b = ctx.scratch_b
        ctx.scratch_b = (None, 0)
        ndir, G, H = w_hh.shape
        gm, params = ctx.gemm, ctx.params
        has_grads = params is not None and all(p.is_leaf and p.grad is not None for ps in params for p in ps)
        if ctx.forms is not None and not has_grads:
            raise RuntimeError('packed_lstm: the forward pass ran on the cached stacked weights (in-place weight gradients), '
                               'but a parameter of the layer has no .grad buffer any more')
        plan = _backward_plan(ctx, lib, x, h0, ndir, H, has_grads, _dc is not None)
        before_recurrence = None
        if _wgrad.pending() and dhy.is_cuda:       # (deferred launches of the layers above: they start where this layer's recurrence starts)
            before_recurrence = torch.cuda.Event()
            before_recurrence.record(torch.cuda.current_stream(dhy.device))
        job = _WgradJob(ctx, lib, plan, x, hy, h0, ndir, H)
        dhy = dhy.contiguous()
        w_t = ctx.forms.w_t if ctx.forms is not None else w_hh.transpose(1, 2).contiguous()      # [ndir, H, 4H]
        if PERSISTENT:
            _watchdog.arm(dhy.device)
        # gradient w.r.t. the FINAL cell state: `_dc` is the gradient of the cell-state tensor this layer returned; packed_lstm
        # exposes only each sequence's last row of it (c_n), so only those rows can carry a gradient: gathered into [ndir, B, H]
        # and handed to the kernel, which adds it to the cell-state gradient at each sequence's last step
        dcn = None
        if _dc is not None and h0 is not None:
            dcv = _dc.reshape(meta.rows, ndir, H)
            dcn = torch.stack([dcv[meta.last_rows[d], d] for d in range(ndir)]).contiguous()
        if plan.state_grad and not (PERSISTENT and lib.ptmi_lstm_split_enabled()):
            raise NotImplementedError('gradients w.r.t. the LSTM states need the persistent split kernels')
        saved = (gates, c, c0, dhy, w_t)
        done = _backward_planes(lib, meta, plan, job, saved, scratch_b, pre_b, ndir, G, H) if plan.use_tp else None
        if done is None and (plan.chunks > 1 or plan.state_grad):
            done = _backward_ranges(lib, meta, plan, job, saved, scratch_b, pre_b, ndir, G, H, dcn)
        if done is None:
            done = _backward_one_call(meta, plan, saved, scratch_b, pre_b, ndir, H)
        dg, dg_t, flags, carry, todo = done
        db_kernel = amax_kernel = None
        if flags is not None:
            if CHECK_PERSISTENT_ERRORS:
                check_errors()
            db_kernel, word = _scratch_tail(lib, flags, meta, ndir, G)
            if lib.ptmi_lstm_split_enabled():
                amax_kernel = word
        flush_pending_wgrad(before_recurrence)          # (captured steps: the layer above's weight gradients, behind this layer's recurrence launch)
        # one scale for the whole gate-gradient tensor (both directions): the backward kernel tracked its maximum
        amax_dg = None if gm is None else amax_kernel if (amax_kernel is not None or dg is None) else _gemm.absmax(dg)
        dx = _input_grad(ctx, lib, plan, dg, flags, amax_dg, amax_kernel, w_ih, ndir, H)
        gh0 = gc0 = None
        if plan.in_place:
            job.finish(dg, dg_t, todo, amax_dg, db_kernel)
            if plan.state_grad:
                gh0, gc0 = _state_grads(meta, dg, w_hh, carry, ndir, G, ctx.needs_input_grad)
            return (dx, None, None, None, None, gh0, gc0) + (None,) * 8
        db = dg.sum(0) if db_kernel is None else db_kernel
        if gm is not None:
            dw_ih = _gemm.mm(dg.t(), x, amax_x=amax_dg, amax_y=gm[0])
            dw_hh = torch.stack([_gemm.mm(a.t(), b, amax_x=amax_dg, amax_y=_gemm.UNIT_RANGE if h0 is None else None)
                                 for a, b in _recurrent_operands(meta, dg, hy, ctx.ext, h0, ndir, H)])
        else:
            dw_ih = dg.t() @ x                                            # [ndir*4H, I]
            dw_hh = torch.stack([a.t() @ b for a, b in _recurrent_operands(meta, dg, hy, ctx.ext, h0, ndir, H)])
        if plan.state_grad:
            gh0, gc0 = _state_grads(meta, dg, w_hh, carry, ndir, G, ctx.needs_input_grad)
        return (dx, dw_ih, db, dw_hh, None, gh0, gc0) + (None,) * 8


def _state_grads(meta, dg, w_hh, carry, ndir, G, needs):
    """Gradients w.r.t. (h0, c0) ``[ndir, B, H]``: ``h0`` entered the pre-activations of each sequence's first processed step
    through ``W_hh`` (``dh0 = dgates_first W_hh``), ``c0`` through that step's forget gate (the kernel's cell-state gradient
    behind its last step)."""
    dgv = dg.view(meta.rows, ndir, G)
    gh0 = torch.stack([dgv[meta.first_rows[d], d] @ w_hh[d] for d in range(ndir)]) if needs[5] else None
    gc0 = carry.clone() if needs[6] else None
    return gh0, gc0


def _recurrent_operands(meta, dg, hy, ext, h0, ndir, H):
    """Per direction d the operands (a, b) of dW_hh[d] = a^T @ b: the gate gradients of every row and the
    hidden state that row's step consumed (zero / h0 for a sequence's first processed step)."""
    rows, G = meta.rows, 4 * H
    dgv = dg.view(rows, ndir, G) if dg is not None else None
    if ext is not None:             # equal lengths: the padded buffer of the forward pass, shifted by one step
        n0 = meta.bs0
        extv = ext.view(rows + 2 * n0, ndir, H)
        return [(dgv[:, d] if dgv is not None else None, extv[:rows, 0] if d == 0 else extv[2 * n0:, 1]) for d in range(ndir)]
    parts = [hy.view(rows, ndir, H), hy.new_zeros(1, ndir, H)]      # row `rows` = zero state
    prev = meta.prev_dev
    if h0 is not None:                                              # rows rows+1+b = h0[:, b]
        parts.append(h0.transpose(0, 1))
        prev = meta.prev_h0_dev
    hy_pad = torch.cat(parts, 0)
    return [(dgv[:, d] if dgv is not None else None, hy_pad[:, d].index_select(0, prev[d])) for d in range(ndir)]


def unsupported_reason(lstm, data):
    """Why :func:`packed_lstm` cannot evaluate ``lstm`` on ``data`` (``None``: it can).  Any ``hidden_size`` and ``bias=False`` are
    covered (round 5: :class:`_PaddedLstm`); ``proj_size`` and non-fp32 modules are not."""
    if not isinstance(lstm, (torch.nn.LSTM, _PaddedLstm)):
        return f'{type(lstm).__name__} is not a torch.nn.LSTM'
    if lstm.proj_size != 0:
        return 'proj_size != 0'
    if not data.is_cuda:
        return 'the input is not on the GPU'
    if data.dtype != torch.float32:
        return f'input dtype {data.dtype} (fp32 only)'
    return None


def supported(lstm, data):
    return unsupported_reason(lstm, data) is None


class _PaddedLstm:
    """A ``torch.nn.LSTM`` whose ``hidden_size`` is not a multiple of 4 (the kernels' unit granularity: 16-byte weight rows), or that has
    no biases, as the LSTM the kernels DO run: every gate block of every parameter zero-padded from H to H4 = 4 ceil(H / 4) units (the
    reference constructs ``torch.nn.LSTM(F, units)`` for any ``units``, ``pit/model.py:60-66``).  A padded unit's pre-activations are 0 at
    every step - i = f = o = 1/2, g = 0, so c = h = 0 for ever - and its columns of ``W_hh`` / of the next layer's ``W_ih`` are zero:
    the real units compute what they compute in the unpadded LSTM, bit for bit in exact arithmetic.  The padded tensors are functions of
    the module's parameters (``F.pad``): gradients reach the parameters through autograd, the padding's gradients are dropped there."""
    proj_size = 0
    bias = True

    def __init__(self, lstm):
        H, ndir = lstm.hidden_size, 2 if lstm.bidirectional else 1
        H4 = (H + 3) // 4 * 4
        self.real_hidden, self.hidden_size = H, H4
        self.num_layers, self.bidirectional, self.dropout, self.training = lstm.num_layers, lstm.bidirectional, lstm.dropout, lstm.training
        ctx = lstm.__dict__.get(_context._ATTR)
        if ctx is not None:
            self.__dict__[_context._ATTR] = ctx
        pad = torch.nn.functional.pad

        def gate_rows(w):                     # [4 H, ...] -> [4 H4, ...]: every gate block padded
            w4 = w.reshape(4, H, *w.shape[1:])
            return pad(w4, (0, 0) * (w4.dim() - 2) + (0, H4 - H)).reshape(4 * H4, *w.shape[1:])
        for layer in range(lstm.num_layers):
            for sfx in (['', '_reverse'] if lstm.bidirectional else ['']):
                w_ih = getattr(lstm, f'weight_ih_l{layer}{sfx}')
                w_hh = getattr(lstm, f'weight_hh_l{layer}{sfx}')
                if layer > 0:                 # the input is the padded output of the layer below: [.., ndir, H4]
                    w_ih = pad(w_ih.reshape(4 * H, ndir, H), (0, H4 - H)).reshape(4 * H, ndir * H4)
                setattr(self, f'weight_ih_l{layer}{sfx}', gate_rows(w_ih))
                setattr(self, f'weight_hh_l{layer}{sfx}', gate_rows(pad(w_hh, (0, H4 - H))))
                for name in ('bias_ih', 'bias_hh'):
                    b = getattr(lstm, f'{name}_l{layer}{sfx}') if lstm.bias else w_hh.new_zeros(4 * H)
                    setattr(self, f'{name}_l{layer}{sfx}', gate_rows(b))


def _packed_lstm_padded(lstm, packed, training, hx, return_state, meta):
    """:func:`packed_lstm` for a module :class:`_PaddedLstm` covers: run the padded LSTM, slice the real units out."""
    shadow = _PaddedLstm(lstm)
    H, H4 = shadow.real_hidden, shadow.hidden_size
    ndir = 2 if lstm.bidirectional else 1
    if hx is not None:
        hx = tuple(torch.nn.functional.pad(t, (0, H4 - H)) for t in hx)
    out = packed_lstm(shadow, packed, training=lstm.training if training is None else training, hx=hx, return_state=return_state, meta=meta)
    states = None
    if return_state or hx is not None:          # (a PackedSequence is a tuple itself: ask what was asked for)
        out, states = out
        states = tuple(t[..., :H] for t in states)
    rows = out.data.shape[0]
    data = out.data.view(rows, ndir, H4)[:, :, :H].reshape(rows, ndir * H)
    out = PackedSequence(data, out.batch_sizes)
    return out if states is None else (out, states)


def packed_lstm(lstm: torch.nn.LSTM, packed: PackedSequence, training=None, hx=None, return_state=False, input_planes=None, meta=None):
    """``lstm(packed, hx)`` through the HIP recurrence.

    ``input_planes = (planes, scale value)``: ``packed.data`` once more as fp16 (hi, lo) planes in the layout of
    ``ptmi_pack_planes_n`` (written by the producer of the data, e.g. ``ops.pit_features``), with the float whose exponent gives
    their operand scale (``ops.gemm.scale_word``): the first layer's projection takes them as they lie.

    ``hx = (h_0, c_0)``, each ``[num_layers * num_directions, B, H]`` like ``torch.nn.LSTM``; gradients flow into the initial
    state and back from the final one ``(h_n, c_n)`` (persistent split kernels).  Returns the output PackedSequence, or
    ``(output, (h_n, c_n))`` when ``hx`` is given or ``return_state`` is set.
    """
    data = packed.data
    _lib.require_gpu(data)
    if not supported(lstm, data):
        raise NotImplementedError('packed_lstm needs an fp32 torch.nn.LSTM with proj_size=0: ' + str(unsupported_reason(lstm, data)))
    if isinstance(lstm, torch.nn.LSTM) and (lstm.hidden_size % 4 != 0 or not lstm.bias):
        # (a producer's fp16 planes of the input - ops.pit_features - are not used on this path: the padded first layer packs its input)
        return _packed_lstm_padded(lstm, packed, training, hx, return_state, meta)
    assert packed.sorted_indices is None, 'sequences must be sorted by length (enforce_sorted=True)'
    training = lstm.training if training is None else training
    oc = _context.effective(lstm)
    if meta is None:
        meta = pack_meta(packed.batch_sizes, data.device)
    else:       # a row-slot layout (ops.sequence.SlotLayout.meta): rows = [T, slots], several sequences end to end per slot
        assert meta.rows == data.shape[0] and hx is None and not return_state and input_planes is None, 'row-slot batches: plain calls only'
        if not (PERSISTENT and _lib.load().ptmi_lstm_split_enabled()):
            raise NotImplementedError('row-slot batches need the persistent split recurrence kernels')
    sfx = ['', '_reverse'] if lstm.bidirectional else ['']
    ndir, H = len(sfx), lstm.hidden_size
    want_state = return_state or hx is not None
    if hx is not None:
        h_all, c_all = hx
        assert h_all.shape == c_all.shape == (lstm.num_layers * ndir, meta.max_batch, H), (h_all.shape, meta.max_batch)
    h_n, c_n = [], []
    h = data.contiguous()
    all_params = [tuple((getattr(lstm, f'weight_ih_l{layer}{s}'), getattr(lstm, f'weight_hh_l{layer}{s}'),
                         getattr(lstm, f'bias_ih_l{layer}{s}'), getattr(lstm, f'bias_hh_l{layer}{s}')) for s in sfx)
                  for layer in range(lstm.num_layers)]
    forked, pre0 = _forms.fork_preparation(all_params, data, H, oc.defer_wgrad, DX_FROM_HANDOFF)
    prev_handoff = None
    for layer in range(lstm.num_layers):
        params = all_params[layer]
        # no graph, or weight gradients accumulated in place by the backward pass (the Trainer's flat bucket): the layer
        # runs on the cached stacked / padded / transposed forms of its parameters
        graph = torch.is_grad_enabled() and any(p.requires_grad for ps in params for p in ps)
        in_place = oc.defer_wgrad and all(p.requires_grad and p.is_leaf and p.grad is not None for ps in params for p in ps)
        forms = anchor = None
        if data.is_cuda and (not graph or in_place):
            forms = _forms.stacked_weights(params, _forms.kpad_of(H), DX_FROM_HANDOFF)
            if forms.ready is not None:
                torch.cuda.current_stream(data.device).wait_event(forms.ready)
            w_ih, bias, w_hh = forms.w_ih, forms.bias, forms.w_hh
            anchor = params[0][0] if graph else None
        else:
            w_ih = torch.cat([ps[0] for ps in params], 0)
            bias = torch.cat([ps[2] + ps[3] for ps in params], 0)
            w_hh = torch.stack([ps[1] for ps in params], 0)
        if want_state:
            sl = slice(layer * ndir, (layer + 1) * ndir)
            h0 = hx[0][sl] if hx is not None else data.new_zeros(ndir, meta.max_batch, H)
            c0 = hx[1][sl] if hx is not None else data.new_zeros(ndir, meta.max_batch, H)
            if oc.grad_use_hook is not None and graph and in_place:
                oc.grad_use_hook([p for ps in params for p in ps])
            h, c = _LstmLayerFn.apply(h, w_ih, bias, w_hh, meta, h0, c0, params, layer > 0, anchor, forms, None, None, False, oc)
            prev_handoff = None
            # (h_n / c_n keep their graph, like torch.nn.LSTM's: the gradient of h_n joins this layer's output gradient, that of c_n
            #  reaches the backward kernel through `c`; modules.StatefulLSTM detaches what it carries between calls)
            hv, cv = h.view(meta.rows, ndir, H), c.view(meta.rows, ndir, H)
            h_n += [hv[meta.last_rows[d], d] for d in range(ndir)]
            c_n += [cv[meta.last_rows[d], d] for d in range(ndir)]
        else:
            out_handoff = {}
            if oc.grad_use_hook is not None and graph and in_place:
                oc.grad_use_hook([p for ps in params for p in ps])
            if layer == 0 and input_planes is not None and prev_handoff is None:
                prev_handoff = {'xplanes': input_planes}
            h = _LstmLayerFn.apply(h, w_ih, bias, w_hh, meta, None, None, params, layer > 0, anchor, forms, prev_handoff, out_handoff,
                                   layer + 1 == lstm.num_layers, oc)
            prev_handoff = out_handoff
        if lstm.dropout > 0 and training and layer + 1 < lstm.num_layers:
            h = torch.nn.functional.dropout(h, lstm.dropout, True)
            prev_handoff = None               # the next layer's input is no longer this layer's output
    _forms.join_preparation(data.device, forked, pre0)
    if not (torch.is_grad_enabled() and h.requires_grad):
        # inference: nobody will run Trainer.clip_grad (which reads the watchdog words of the persistent kernels during
        # training) - check them here, so that results of a timed-out launch are never returned silently
        check_errors()
    if prev_handoff and prev_handoff.get('planes') is not None:
        # the recurrence has left this very tensor as fp16 planes too: ops.linear takes them as operand A when it is handed the SAME
        # tensor object, unmodified (the record travels WITH the tensor - until round 3 it was a process global naming "the last
        # call's output", a side channel between two ops that two models or two host threads would have shared)
        setattr(h, HANDOFF_ATTR, (h._version, prev_handoff['planes'], ndir, H))
    out = PackedSequence(h, packed.batch_sizes)
    if want_state:
        return out, (torch.stack(h_n), torch.stack(c_n))
    return out
