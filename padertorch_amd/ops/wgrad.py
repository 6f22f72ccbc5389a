"""The weight-gradient queue: where ``ops.lstm`` and ``ops.linear`` accumulate weight gradients in place, beside the recurrences.

Contract:

* :func:`stream` is THE side stream of the current main stream; work on it is ordered by its user (``side.wait_stream(main)`` or
  an event) and joined by :func:`sync_deferred`, which must run before anything reads the gradients (the Trainer does).
* :func:`defer` parks a launch closure ``fn(start)`` until the next lower BLSTM layer's recurrence has been enqueued
  (:func:`flush_pending`, also called by :func:`sync_deferred`); :func:`abandon` drops the parked closures of a step that failed.
* :func:`mark_done` / :func:`wait_done`: the event behind the last side-stream accumulation into a parameter's ``.grad``.
* :func:`reset_step` forgets the events of earlier steps (``ops.capture.reset_step_caches``).

Only shapes for which :func:`gemm_keys_safe` holds (or kernels that never wait for sibling workgroups) may run on the side stream
next to a persistent recurrence kernel: see ``ops.lstm.DEFER_WGRAD``.
"""
import torch

from .. import _lib

_WGRAD_STREAMS = {}
_WGRAD_DONE = {}
#: captured steps (ops.capture): a layer's weight-gradient launches are ENQUEUED behind the next lower layer's recurrence launch (they
#: still wait for the event recorded where they used to be enqueued).  The hipGraph executor lays a captured step out by following a
#: node's FIRST-captured successor on the same queue: with the side-stream chain captured first, the next recurrence ended up behind
#: that chain on one queue (rocprofv3 timeline of the replay: 0.43 ms of weight-gradient GEMMs in front of the first layer's backward
#: recurrence instead of beside it); with the recurrence captured first the chain gets a queue of its own.
_PENDING_WGRAD = []
_SIDE_SAFE = {}


def defer(fn):
    """Park ``fn(start)`` until :func:`flush_pending`."""
    _PENDING_WGRAD.append(fn)


def pending():
    return bool(_PENDING_WGRAD)


def flush_pending(start=None):
    """Enqueue the deferred weight-gradient launches.  ``start``: an event on the main queue that launches without an event of their own
    (``ops.linear``: the dense layers' weight gradients) wait for - recorded in FRONT of the recurrence launch they are enqueued behind,
    i.e. they start beside that recurrence instead of beside the dense layers' input-gradient chain that leads up to it."""
    while _PENDING_WGRAD:
        _PENDING_WGRAD.pop(0)(start)


def abandon():
    """Drop the parked launches (a capture that raised: they name its tensors and events)."""
    del _PENDING_WGRAD[:]


def reset_step():
    _WGRAD_DONE.clear()


def mark_done(params, event):
    for p in params:
        _WGRAD_DONE[id(p)] = event


def wait_done(queue, params):
    """``queue`` waits for the earlier side-stream accumulations into the ``.grad`` views of ``params``."""
    for p in params:
        ev = _WGRAD_DONE.get(id(p))
        if ev is not None:
            queue.wait_event(ev)


# (Measured in round 2 and not kept - DESIGN.md sections 3.9 / 4 have the numbers -: the pattern fill ahead of time on a side stream,
# the weight gradients' forward-data operand planes packed during the forward pass, a layer's weight gradients started behind its
# recurrence instead of behind its input-gradient GEMM, the backward recurrence cut into several launches.)


def stream(device):
    """The weight-gradient side stream that belongs to the CURRENT stream of ``device``: one per (device, main stream), so that
    two host threads that drive their own models on their own streams (reference ``trainer.py:412-420``) do not serialise on, or
    order themselves through, one shared side queue.  (The backward pass runs on autograd's thread with the forward pass' stream
    current, i.e. it finds the forward pass' side stream.)"""
    device = torch.device(device)
    # (keyed by the raw handle: torch hands out stream wrappers afresh on every call, so there is no object to hold weakly.  torch's
    #  streams come from a fixed pool per device and are never destroyed - a handle seen again IS the same queue -, so the table is
    #  bounded by the pool; an external stream that was destroyed and whose handle came back would find its predecessor's side stream,
    #  which is a valid side stream for it too.)
    key = _lib.device_key(device) + (torch.cuda.current_stream(device).cuda_stream,)
    if key not in _WGRAD_STREAMS:
        if len(_WGRAD_STREAMS) >= 64:
            sync_deferred()                     # nothing may be pending on a side stream that is let go
            _WGRAD_STREAMS.clear()
        _WGRAD_STREAMS[key] = torch.cuda.Stream(device=device)
    return _WGRAD_STREAMS[key]


def gemm_keys_safe(keys):
    """True when every TunableOp GEMM key has a pinned rocBLAS solution in the loaded results: rocBLAS
    kernels are plain tiled GEMMs (split-K through a second kernel), hipBLASLt's carry a Stream-K mode
    that spins on sibling workgroups - the latter must not run next to a persistent recurrence kernel
    (see ``ops.lstm.DEFER_WGRAD``).  Unknown shapes run on the main stream."""
    keys = tuple(keys)
    if keys not in _SIDE_SAFE:
        ok = False
        try:
            import torch.cuda.tunable as tunable
            if tunable.is_enabled():
                res = {params: sol for _op, params, sol, _t in tunable.get_results()}
                ok = all('Rocblas' in res.get(k, '') for k in keys)
        except Exception:
            ok = False
        _SIDE_SAFE[keys] = ok
    return _SIDE_SAFE[keys]


def wgrad_key(n_in, n_out, rows, ld_g=None, ld_x=None):
    """TunableOp key of ``W.grad[n_out, n_in].addmm_(g[rows, n_out].t(), x[rows, n_in])`` (``ld_g`` / ``ld_x``:
    row strides of ``g`` / ``x`` when they are column blocks of wider matrices)."""
    return f'nt_{n_in}_{n_out}_{rows}_ld_{ld_x or n_in}_{ld_g or n_out}_{n_in}'


def warm_side_stream(device, nbytes=1 << 30):
    """Create the weight-gradient side stream of ``device`` and exercise everything it will need (its
    hardware queue, the allocator pool of that stream, the BLAS handle, the kernels) while the GPU is
    otherwise IDLE.  First use of a stream next to a running persistent recurrence kernel has been
    observed to stall the GPU (queue creation / first large allocations while a kernel that needs all of
    its workgroups co-resident is only partly dispatched); after this warm-up it does not."""
    device = torch.device(device)
    torch.cuda.synchronize(device)
    side = stream(device)
    with torch.cuda.stream(side):
        big = torch.empty(nbytes // 4, dtype=torch.float32, device=device)      # grows the side pool once
        a = torch.randn(512, 256, device=device)
        idx = torch.arange(512, device=device)
        acc = torch.zeros(256, 256, device=device)
        acc.addmm_(a.t(), torch.cat([a, a[:1]], 0).index_select(0, idx))
        acc.add_(a.sum(0))
        del big, a, idx, acc
    torch.cuda.synchronize(device)


def sync_deferred(device=None):
    """Make the current stream wait for every deferred weight-gradient accumulation."""
    flush_pending()
    want = _lib.device_key(device) if device is not None else None
    from . import capture as _capture
    for (typ, idx, main_handle), side in list(_WGRAD_STREAMS.items()):
        if want is None or want == (typ, idx):
            cur = torch.cuda.current_stream(torch.device(typ, idx))
            if _capture.ACTIVE and main_handle != cur.cuda_stream:
                continue            # a captured step joins ITS side stream; a wait for a stream outside the capture is no edge of the graph
            cur.wait_stream(side)
