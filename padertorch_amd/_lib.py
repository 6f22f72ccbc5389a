"""ctypes binding of libptmi.so (C ABI declared in include/ptmi.h).

The product path has NO CPU fallback: if the library is missing, or a tensor is not on an
MI355X device, the ops raise instead of silently computing something else.
"""
import ctypes
import os
import threading
from ctypes import c_int, c_int32, c_int64, c_void_p
from pathlib import Path

import torch

from . import _capi

_PKG = Path(__file__).resolve().parent
LIB_PATH = _PKG / 'libptmi.so'
if os.environ.get('PTMI_LIB'):            # A/B runs against another build of the same ABI (experiments only)
    LIB_PATH = Path(os.environ['PTMI_LIB'])

HEADER_PATH = _PKG.parent / 'include' / 'ptmi.h'
if not HEADER_PATH.exists():
    raise ImportError(f'{HEADER_PATH} is missing: the ctypes signatures of libptmi.so are read from the header that declares them.')
_HEADER = HEADER_PATH.read_text()


class StftGeom(ctypes.Structure):
    """``ptmi_stft_geom`` (include/ptmi.h)."""
    _fields_ = _capi.struct_fields(_HEADER, 'ptmi_stft_geom')


class NormGeom(ctypes.Structure):
    """``ptmi_norm_geom`` (include/ptmi.h)."""
    _fields_ = _capi.struct_fields(_HEADER, 'ptmi_norm_geom')


#: name -> (restype, argtypes) of every function include/ptmi.h declares, by the type mapping at the top of ``_capi``
SIGNATURES = _capi.signatures(_HEADER, {'ptmi_stft_geom': StftGeom, 'ptmi_norm_geom': NormGeom})

_lib = None


def load():
    """Load libptmi.so (once).  Raises if it has not been built - there is no fallback."""
    global _lib
    if _lib is None:
        if not LIB_PATH.exists():
            raise ImportError(
                f'{LIB_PATH} is missing: build the HIP kernels first '
                f'(python -m padertorch_amd.build, or __graft_entry__.build()). '
                f'padertorch_amd has no CPU fallback.')
        lib = ctypes.CDLL(str(LIB_PATH))
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(lib, name)          # AttributeError if the symbol is not exported
            fn.restype = res
            fn.argtypes = args
        _lib = lib
    return _lib


_hooks = None


def test_hooks():
    """``libptmi_testhooks.so`` (``csrc/testhooks``: ``ptmi_test_occupy``) - kernels only tests and measurement brackets launch; not part
    of the hot path's library."""
    global _hooks
    if _hooks is None:
        path = _PKG / 'libptmi_testhooks.so'
        if not path.exists():
            raise ImportError(f'{path} is missing: python -m padertorch_amd.build')
        lib = ctypes.CDLL(str(path))
        lib.ptmi_test_occupy.restype = c_int
        lib.ptmi_test_occupy.argtypes = [c_int32, c_int32, c_int32, c_int64, c_void_p]
        _hooks = lib
    return _hooks


def select_gemm_tile(tile):
    """Pin the planes GEMM's workgroup tile for the calls that follow (0..5; -1 / None: the cost model) - the ``PTMI_GEMM_TILE`` variable
    ``csrc/gemm_planes.hip`` reads at every call: tests and sweeps only."""
    if tile is None or tile < 0:
        os.environ.pop('PTMI_GEMM_TILE', None)
    else:
        assert 0 <= tile <= 5, tile
        os.environ['PTMI_GEMM_TILE'] = str(int(tile))
    return 0


def check(rc, what=''):
    if rc != 0:
        msg = load().ptmi_error_string(int(rc)).decode()
        raise RuntimeError(f'{what}: {msg} (code {rc})')


def ptr(t):
    """Device pointer of a tensor (None -> NULL)."""
    return None if t is None else t.data_ptr()


def require_gpu(*tensors):
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise RuntimeError(
                'padertorch_amd ops run on an MI355X (HIP) device only and have no CPU fallback; '
                f'got a tensor on {t.device}. Move the example to the GPU first.')


def stream(device):
    return torch.cuda.current_stream(device).cuda_stream


def device_key(device):
    """``(type, index)`` with the index filled in (``cuda`` -> the current device): the key of every per-GPU registry."""
    device = torch.device(device)
    return device.type, device.index if device.index is not None else torch.cuda.current_device()


#: when a list, ``timed`` brackets every kernel launch with HIP events recorded on the launch stream
#: and appends ``(name, start_event, end_event)`` (bench.py's roofline figure); None = off
KERNEL_TIMERS = None


def timed(name, fn, *args):
    """Call a C-ABI launcher; optionally bracket it with events on torch's current stream."""
    if KERNEL_TIMERS is None:
        return fn(*args)
    e0 = torch.cuda.Event(enable_timing=True)
    e1 = torch.cuda.Event(enable_timing=True)
    e0.record()
    rc = fn(*args)
    e1.record()
    KERNEL_TIMERS.append((name, e0, e1))
    return rc


def call(symbol, *args, timer=None, accept=()):
    """Launch the C-ABI entry point ``symbol`` (``'ptmi_...'``) with ``args``, under :func:`timed` as ``timer`` when one is given, and
    :func:`check` its return code with the symbol as the label.  A code listed in ``accept`` is returned instead of raised: ``(-2,)``
    where PTMI_E_UNSUPPORTED - nothing was enqueued - sends the caller another route."""
    fn = getattr(load(), symbol)
    rc = timed(timer, fn, *args) if timer else fn(*args)
    if rc and rc not in accept:
        check(rc, symbol)
    return rc


class _Staging:
    """Pinned staging memory for small host -> device copies: two halves used in turn.  One event per half (recorded when the half is
    left) says when the copies out of it have run; a half is written again only behind its event - long fired by then.  (A fresh
    ``pin_memory()`` per copy works too, but its allocator has to make a new pinned block whenever the previous step's block is still in
    flight: 70 ms of hipHostMalloc now and then for the 0.5 MB index tables of a 64 x 6 s batch.)"""

    def __init__(self, half_bytes=1 << 24):
        self.half = half_bytes
        self.buf = torch.empty(2 * half_bytes, dtype=torch.uint8, pin_memory=True)
        self.np = self.buf.numpy()            # the same memory for numpy: a plain memcpy fills it (torch's CPU copy_ of > 32 k elements
        #                                       goes through the intra-op thread pool: 0.4 ms and more on a loaded many-core host)
        self.which, self.off = 0, 0
        self.events = [[], []]           # per half: events behind the copies out of it (one per stream that copied)
        self.streams = [{}, {}]          # per half: the streams that have copied out of it since it was entered
        self.lock = threading.Lock()

    def put(self, t, device):
        n = t.numel() * t.element_size()
        if n > self.half // 4:
            return t.pin_memory().to(device, non_blocking=True)
        with self.lock:
            if self.off + n > self.half:                       # leave this half: an event behind everything copied out of it
                for stream in self.streams[self.which].values():
                    ev = torch.cuda.Event()
                    ev.record(stream)
                    self.events[self.which].append(ev)
                self.streams[self.which] = {}
                self.which, self.off = self.which ^ 1, 0
                for ev in self.events[self.which]:
                    ev.synchronize()
                self.events[self.which] = []
            start = self.which * self.half + self.off
            self.off += (n + 63) // 64 * 64
            stage = self.buf[start:start + n].view(t.dtype).view(t.shape)
            self.np[start:start + n] = t.numpy().reshape(-1).view('uint8')
            cur = torch.cuda.current_stream(device)
            self.streams[self.which][cur.cuda_stream] = cur
            return stage.to(device, non_blocking=True)


_STAGING = {}


def host_to_device(values, dtype, device):
    """A small host list / ndarray as a device tensor WITHOUT a host synchronisation: pinned staging memory + non-blocking copy.
    (``torch.tensor(values, device='cuda')`` copies from pageable memory, which blocks the host until the stream has drained: with
    one such call per step - the lengths of a ragged batch - the host never runs ahead of the GPU and every launch gap of the step
    becomes visible: 12.7 instead of 10.0 ms per step for 32 examples of 3-6 s)"""
    t = torch.as_tensor(values, dtype=dtype)
    device = torch.device(device)
    if device.type != 'cuda' or t.numel() == 0:
        return t.to(device)
    idx = device.index if device.index is not None else torch.cuda.current_device()
    st = _STAGING.get(idx)
    if st is None:
        st = _STAGING[idx] = _Staging()
    return st.put(t.contiguous(), torch.device('cuda', idx))


def int64s(*vals):
    """A HOST ``int64_t`` array argument (the stride arrays of include/ptmi.h)."""
    return (c_int64 * len(vals))(*vals)


#: PTMI_STRICT=1 (or ``padertorch_amd._lib.STRICT = True``): a request that would leave the hand-written HIP path - an LSTM the
#: recurrence kernels do not cover, a dense layer handed to the BLAS library - raises instead of warning.  The GPU test suite runs strict.
STRICT = bool(int(os.environ.get('PTMI_STRICT', '0') or 0))
_WARNED = set()


def leaving_native_path(what, reason):
    """``what`` is about to run on a library kernel (MIOpen / rocBLAS through torch) instead of this package's HIP kernels because
    of ``reason``: said once per (what, reason) as a ``RuntimeWarning``, or raised under :data:`STRICT` - never silently."""
    msg = f'padertorch_amd: {what} runs on the torch / library path, not on the HIP kernels: {reason}'
    if STRICT:
        raise RuntimeError(msg + ' (PTMI_STRICT)')
    if (what, reason) not in _WARNED:
        _WARNED.add((what, reason))
        import warnings
        warnings.warn(msg, RuntimeWarning, stacklevel=3)
