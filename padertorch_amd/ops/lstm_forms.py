"""The operand forms of a (B)LSTM layer's parameters, and the queues they are made on.

Contract:

* :func:`stacked_weights` returns the :class:`LayerForms` of one layer, cached until a parameter is modified (``_version`` /
  storage / identity); :func:`clear` drops the cache (``ops.gemm.invalidate``).  A consumer waits for ``forms.ready`` when it is set.
* :func:`fork_preparation` (first thing of ``ops.lstm.packed_lstm``) makes the stale forms of all layers on the preparation queues,
  :func:`join_preparation` (last thing) joins those queues to a capturing stream again.
* :func:`begin_captured_step` / :func:`end_captured_step` bracket the capture of an optimizer step (``train.graphed``);
  :func:`reset_step` forgets a capture's forks (``ops.capture.reset_step_caches``).

The switches of ``ops.lstm`` this module depends on arrive as arguments (``dx_from_handoff``, ``defer_wgrad``).
"""
import torch

from .. import _lib
from . import gemm as _gemm

_STACKED = {}
_PREP_STREAMS = {}
_EARLY_FORK = {}            # (device type, index) -> the preparation streams a captured step has forked at its very start


def clear():
    _STACKED.clear()


def reset_step():
    _EARLY_FORK.clear()


def kpad_of(H):
    """Columns of ``W_hh`` padded to the matrix cores' reduction granularity."""
    return (H + 15) // 16 * 16


def _prep_stream(device, first_layer=False):
    """The parameter-form queue (``first_layer``: a second one, for the first BLSTM layer's forms of a captured step - see
    :func:`begin_captured_step`)."""
    key = _lib.device_key(device) + (bool(first_layer),)
    if key not in _PREP_STREAMS:
        _PREP_STREAMS[key] = torch.cuda.Stream(device=device)
    return _PREP_STREAMS[key]


def begin_captured_step(device):
    """First thing inside the capture of an optimizer step (``train.graphed``, behind ``ops.capture.zero_block``): the preparation
    queue forks HERE - in front of the front-end kernels - instead of at the first BLSTM call, so that a replay makes every parameter
    form (all BLSTM layers', the dense layers' of the earlier steps) NEXT TO the feature kernel instead of behind it.  They read the
    parameters only, which the previous replay's optimizer kernel wrote.  (Round 5's replay: first recurrence at 490 us of the step;
    with this and the shorter ``lstm_weight_prep`` at 280 - of which the step keeps 40-60 us, the forms now run beside the first
    recurrence and slow it: DESIGN 4.4, ``profiles/r6_head_of_step.txt``.)"""
    from . import capture as _capture
    assert _capture.ACTIVE
    device = torch.device(device)
    # (Measured as a three-way switch and fixed: forms made as the eager step orders them - the first layer's on the main queue
    #  behind the feature kernel, the others' on a queue that forks at the first BLSTM call -; the others' queue forked at the head
    #  of the graph; that, and the first layer's forms on a SECOND queue forked there too.  The last is what runs.)
    pre, pre0 = _prep_stream(device), _prep_stream(device, True)
    pre.wait_stream(torch.cuda.current_stream(device))
    pre0.wait_stream(torch.cuda.current_stream(device))
    _EARLY_FORK[_lib.device_key(device)] = (pre, pre0)
    # (Only the forks: the work itself is enqueued where it always was, by the first BLSTM call - a replay submits its nodes in
    #  capture order, and with the forms captured FIRST the feature kernel, head of the critical path, started 170 us later.  Two
    #  queues: a replay runs the nodes of one captured stream in order, and the first projection - whose operands are the feature
    #  kernel's output and the FIRST layer's forms - landed on the form queue behind all the other layers' forms, at 350 us.)


def end_captured_step(device):
    """Last thing inside the capture: every side queue the step has forked joins the capturing stream."""
    device = torch.device(device)
    for side in _EARLY_FORK.pop(_lib.device_key(device), ()):
        torch.cuda.current_stream(device).wait_stream(side)


def _stacked_stale(params):
    flat = tuple(p for ps in params for p in ps)
    hit = _STACKED.get(tuple(id(p) for p in flat))
    return hit is None or hit[0] != tuple((p._version, p.data_ptr()) for p in flat) or not _gemm._same(hit[2], flat)


class _LazyPlanes:
    """``ops.gemm.pack_n(w, amax)`` on first use (on the stream current then; ``w`` and ``amax`` were written on the stream the
    forms were made on, whose ``ready`` event every consumer has waited for)."""

    def __init__(self, w, amax):
        self.w, self.amax, self.value = w, amax, None

    def get(self):
        if self.value is None:
            with torch.no_grad():
                self.value = _gemm.pack_n(self.w, self.amax)
        return self.value


class LayerForms:
    """Both directions' parameters of one layer as the kernels take them.  ``w_ih`` ``[ndir 4H, I]`` stacked, ``bias`` the summed
    biases, ``w_hh`` ``[ndir, 4H, H]``, ``w_pad`` the same padded to ``KP`` columns, ``w_t`` transposed, ``w_ih_kpad`` ``w_ih`` with
    the reduction axis zero-padded to a multiple of 4 (``None``: it is one).  Kernel path only, ``None`` otherwise: ``ready`` (event
    behind the forms when they were made on a preparation stream), ``w_ih_planes`` (fp16 planes of ``w_ih``, read through
    :meth:`input_planes`), ``w_ih_planes_h`` ``((planes, amax), cols)`` (the same laid out like the previous layer's hand-off
    planes), ``w_ih_planes_dx`` ``(planes, cols)`` (bf16 planes for ``dx = dgates W_ih``)."""

    def __init__(self, w_ih, bias, w_hh, w_pad, w_t, w_ih_kpad, w_ih_planes=None, w_ih_planes_h=None, w_ih_planes_dx=None):
        self.w_ih, self.bias, self.w_hh, self.w_pad, self.w_t, self.w_ih_kpad = w_ih, bias, w_hh, w_pad, w_t, w_ih_kpad
        self.w_ih_planes, self.w_ih_planes_h, self.w_ih_planes_dx = w_ih_planes, w_ih_planes_h, w_ih_planes_dx
        self.ready = None

    def input_planes(self):
        v = self.w_ih_planes
        return v.get() if isinstance(v, _LazyPlanes) else v


def _forms_kernel(params, KP, dx_from_handoff, stream):
    """One launch: every parameter is read once (csrc/lstm_prep.hip); on ``stream`` when the caller prefetches the forms of later
    layers next to the first layer's work (consumers wait for ``forms.ready``)."""
    p0 = params[0][0]
    main = torch.cuda.current_stream(p0.device)
    with torch.cuda.stream(stream if stream is not None else main):
        w_ih_k, bias, w_pad, w_t, amax = torch.ops.ptmi.lstm_weight_prep(
            [ps[0].detach() for ps in params], [ps[1].detach() for ps in params], [ps[2].detach() for ps in params],
            [ps[3].detach() for ps in params], KP)
        I, H = p0.shape[1], params[0][1].shape[1]
        # the stacked input weights with their input columns laid out like the previous layer's hand-off planes (H columns
        # per direction padded to the planes' width): that layer's scratch then is operand A of this layer's projection
        planes = planes_h = None
        ndir_ = len(params)
        cols_ = int(_lib.load().ptmi_lstm_handoff_cols(H, 0)) if _gemm.planes_enabled() else 0
        if cols_ and I == ndir_ * H:
            planes_h = ((_gemm.pack_n_direction_blocks(w_ih_k[:, :I], ndir_, H, cols_, amax[0:1]), amax[0:1]), cols_)
            if cols_ == H:
                planes = planes_h[0]
        # fp16 planes of the stacked input weights as they are (the W of x W^T on csrc/gemm_planes.hip): at once for a
        # layer that has no other form (the first: its input is no hidden state), on first use (a dropout between the
        # layers, an initial state) for the others
        if _gemm.planes_enabled() and planes is None:
            planes = _gemm.pack_n(w_ih_k[:, :I], amax[0:1]) if planes_h is None else _LazyPlanes(w_ih_k[:, :I], amax[0:1])
        # bf16 planes of W_ih as the right operand of dx = dgates W_ih on the backward recurrence's planes (layers whose
        # input needs a gradient: not the first); built here, off the backward pass' critical path
        planes_dx = None
        cols_b = int(_lib.load().ptmi_lstm_handoff_cols(H, 1)) if (planes is not None and dx_from_handoff) else 0
        if cols_b and I == ndir_ * H:
            planes_dx = (_gemm.stacked_planes_t_bf16(w_ih_k[:, :I], ndir_, cols_b), cols_b)
    forms = LayerForms(w_ih_k[:, :I], bias, w_pad[:, :, :H], w_pad, w_t, w_ih_k if w_ih_k.shape[1] != I else None,
                       planes, planes_h, planes_dx)
    if stream is not None:
        forms.ready = torch.cuda.Event()
        forms.ready.record(stream)
        # These tensors come from the preparation stream's pool and are read on the main stream.  They are NOT marked with
        # record_stream(main): the allocator would then record one event per tensor on the MAIN queue when they are freed
        # (20 marker packets = a 75 us bubble behind the top layer's recurrence, where the previous step's graph let go
        # of them: scripts/phase_events.py, rocprofv3 --hip-runtime-trace).  Their memory can only be handed out again
        # by an allocation on the preparation stream, and every piece of work on that stream is enqueued behind a wait
        # for the optimizer kernel / the main stream (fork_preparation), i.e. behind every reader of the old forms.
    _gemm.seed_weights_absmax([ps[0] for ps in params], amax[0:1])
    _gemm.seed_weights_absmax([ps[1] for ps in params], amax[1:2])
    return forms


def _forms_torch(params, KP):
    """The same forms by torch ops (CPU tensors, non-fp32 or non-contiguous parameters)."""
    w_ih = torch.cat([ps[0] for ps in params], 0)
    bias = torch.cat([ps[2] + ps[3] for ps in params], 0)
    w_hh = torch.stack([ps[1] for ps in params], 0)
    H = w_hh.shape[2]
    kpad = -w_ih.shape[1] % 4
    # (keyword order = evaluation order of the forms' kernels)
    return LayerForms(
        w_ih=w_ih, bias=bias, w_hh=w_hh,
        w_ih_kpad=torch.nn.functional.pad(w_ih, (0, kpad)) if kpad else None,
        w_pad=torch.nn.functional.pad(w_hh, (0, KP - H)).contiguous() if KP != H else w_hh.contiguous(),
        w_t=w_hh.transpose(1, 2).contiguous())


def stacked_weights(params, KP, dx_from_handoff, stream=None):
    """The per-layer operand forms of a BLSTM layer's parameters - both directions' ``weight_ih`` stacked (and, for an
    input width that is not a multiple of 4, zero-padded along the reduction axis), the summed biases, ``weight_hh``
    stacked, padded to ``KP`` columns and transposed - cached until a parameter is modified (``_version`` / storage):
    they change once per optimizer step, not per micro-step or layer call (six concatenation / padding / transposition
    kernels per layer and pass, ~70 us of launch-bound work per layer of the B = 32 step).  Detached: only for calls
    whose weight gradients do not travel through autograd (``DEFER_WGRAD`` path, or no graph at all)."""
    key = tuple(id(p) for ps in params for p in ps)
    sig = tuple((p._version, p.data_ptr()) for ps in params for p in ps)
    flat_ps = tuple(p for ps in params for p in ps)
    hit = _STACKED.get(key)
    if hit is not None and hit[0] == sig and _gemm._same(hit[2], flat_ps):      # (weak references: see ops.gemm._WEIGHT_AMAX)
        return hit[1]
    if len(_STACKED) > 64:
        _STACKED.clear()
    with torch.no_grad():
        if params[0][0].is_cuda and all(p.dtype == torch.float32 and p.is_contiguous() for ps in params for p in ps):
            forms = _forms_kernel(params, KP, dx_from_handoff, stream)
        else:
            forms = _forms_torch(params, KP)
    _STACKED[key] = (sig, forms, _gemm._refs(flat_ps))
    return forms


def fork_preparation(all_params, data, H, defer_wgrad, dx_from_handoff):
    """After an optimizer step: the operand forms of ALL layers on a side stream, next to whatever the main stream is doing (the
    front-end kernels, the first projection), instead of one launch in front of every layer's projection.  ``all_params``: per
    layer, per direction ``(w_ih, w_hh, b_ih, b_hh)``; ``data``: the LSTM's input.  Returns the queues :func:`join_preparation`
    takes: ``(forked, pre0)``, both ``None`` when nothing was forked."""
    flat_params = [p for ps_ in all_params for ps in ps_ for p in ps]
    if not (data.is_cuda and any(_stacked_stale(ps_) for ps_ in all_params)
            and all(p.is_cuda and p.dtype == torch.float32 for p in flat_params)
            and (not (torch.is_grad_enabled() and any(p.requires_grad for p in flat_params))
                 or (defer_wgrad and all(p.requires_grad and p.is_leaf and p.grad is not None for p in flat_params)))):
        return None, None
    pre = _prep_stream(data.device)
    updated = _gemm.update_event(flat_params)
    from . import capture as _capture
    early = _EARLY_FORK.get(_lib.device_key(data.device)) if _capture.ACTIVE else None
    pre0 = early[1] if early else None
    early = bool(early)
    if early:
        pass                          # a captured step: forked at the head of the graph (begin_captured_step), nothing to wait for
    elif updated is not None:
        pre.wait_event(updated)       # behind the optimizer kernel, i.e. next to the step's front-end, not behind it
    else:
        pre.wait_stream(torch.cuda.current_stream(data.device))
    for layer, ps_ in enumerate(all_params):
        # (the first layer's too in a captured step: a cross-queue edge of a graph costs no host time)
        if _stacked_stale(ps_) and (layer > 0 or pre0 is not None):
            stacked_weights(ps_, kpad_of(H), dx_from_handoff, stream=pre if layer > 0 else pre0)
    if updated is not None or early:
        with torch.cuda.stream(pre):
            _gemm.prefetch_known(data.device, everything=early)       # the dense layers' operand forms of the last steps, behind them
    # the first layer's forms are needed at once: on the main queue itself (a cross-queue wait in front of the first
    # projection was measured to cost the main queue 110-260 us; the later layers' forms are long done when their
    # projection is reached, and a wait for a finished event costs nothing)
    return pre, pre0


def join_preparation(device, forked, pre0):
    """A captured step: the preparation stream has forked from the capturing stream (:func:`fork_preparation`) and must join it
    again, whether or not a layer has waited for its forms (by now they are long done: the wait is free)."""
    from . import capture as _capture
    if _capture.ACTIVE and forked is not None:
        torch.cuda.current_stream(device).wait_stream(forked)
        if pre0 is not None:
            torch.cuda.current_stream(device).wait_stream(pre0)
