"""The C-ABI library loads and exports every symbol include/ptmi.h declares (no GPU needed)."""
import ctypes
import re
from pathlib import Path

import pytest

REPO = Path(__file__).resolve().parent.parent


def declared_symbols():
    text = (REPO / 'include' / 'ptmi.h').read_text()
    text = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    return sorted(set(re.findall(r'\b(ptmi_[a-z0-9_]+)\s*\(', text)))


def test_library_exports_header():
    from padertorch_amd import _lib
    from padertorch_amd.build import build
    build()
    lib = ctypes.CDLL(str(_lib.LIB_PATH))
    syms = declared_symbols()
    assert len(syms) >= 10
    for s in syms:
        assert hasattr(lib, s), f'{s} declared in ptmi.h but not exported'
    assert set(syms) == set(_lib.SIGNATURES), set(syms) ^ set(_lib.SIGNATURES)
    _lib.load()


def test_frame_bookkeeping_is_bit_exact(g1, g2):
    """ptmi_stft_num_frames / ptmi_istft_num_samples: integer parity with the reference."""
    from padertorch_amd import _lib
    from padertorch_amd.ops import STFT
    lib = _lib.load()
    for fc in g1['frame_counts']:
        st = STFT(fc['size'], fc['shift'], window_length=fc['window_length'], fading=fc['fading'])
        for n, fr in zip(fc['samples'], fc['frames']):
            assert lib.ptmi_stft_num_frames(st._geom, n) == fr == st.samples_to_frames(n)
    for c in g2['cases']:
        st = STFT(c['size'], c['shift'], window=c['window'], window_length=c['window_length'],
                  fading=c['fading'], pad=c['pad'])
        n = g2[c['x']].shape[-1]
        assert lib.ptmi_stft_num_frames(st._geom, n) == c['frames'] == st.samples_to_frames(n)
        assert lib.ptmi_istft_num_samples(st._geom, c['frames']) == c['samples_back'] \
            == st.frames_to_samples(c['frames'])


def test_no_cpu_fallback():
    import torch
    from padertorch_amd.ops import STFT, pit_loss
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        STFT(512, 128)(torch.zeros(2, 1000))
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        pit_loss(torch.zeros(4, 2, 5), torch.zeros(4, 2, 5), axis=1)


def test_stft_argument_checks():
    from padertorch_amd.ops import STFT
    with pytest.raises(AssertionError, match='even FFT sizes'):
        STFT(511, 128)
    with pytest.raises(AssertionError):
        STFT(512, 128, complex_representation='polar')
    with pytest.raises(AssertionError):
        STFT(512, 128, fading='quarter')


def test_kernels_are_registered_torch_ops_without_a_cpu_kernel():
    """The hot-path kernels are torch custom ops (torch.ops.ptmi.*) over the C ABI; they have a CUDA kernel only."""
    import torch
    import padertorch_amd  # noqa: F401  (registers the library)
    names = {'stft_forward', 'istft_forward', 'pit_features', 'pit_loss_forward', 'pit_loss_backward', 'dc_loss_forward',
             'dc_loss_backward', 'unit_norm_forward', 'unit_norm_backward', 'lstm_recurrence_forward',
             'lstm_recurrence_backward', 'absmax', 'gemm_planes_', 'pack_planes_n', 'pack_planes_t', 'pit_features_packed'}
    for n in names:
        op = getattr(torch.ops.ptmi, n)
        assert op.default._schema.name == f'ptmi::{n}'
        assert torch._C._dispatch_has_kernel_for_dispatch_key(f'ptmi::{n}', 'CUDA')
        assert not torch._C._dispatch_has_kernel_for_dispatch_key(f'ptmi::{n}', 'CPU')
    assert torch.ops.ptmi.gemm_planes_.default._schema.arguments[0].alias_info.is_write     # out is written in place
    with pytest.raises(NotImplementedError):
        torch.ops.ptmi.absmax(torch.ones(2, 2), 2, 2, 2)                                    # CPU tensor: no kernel, no fallback


def test_signatures_are_the_headers():
    """A handful of signatures and both structures written out in full: one per rule of the header -> ctypes mapping."""
    from ctypes import POINTER, c_char_p, c_double, c_float, c_int, c_int32, c_int64, c_void_p, sizeof
    from padertorch_amd import _lib
    P, G, N = c_void_p, POINTER(_lib.StftGeom), POINTER(_lib.NormGeom)
    pinned = {
        'ptmi_version': (c_char_p, []),
        'ptmi_error_string': (c_char_p, [c_int]),
        'ptmi_stft_num_frames': (c_int64, [G, c_int64]),
        'ptmi_stft_forward': (c_int, [P, c_int64, c_int64, c_int64, P, P, P, G, c_int64, c_int32, c_float, P, P]),
        'ptmi_norm_reduce': (c_int, [c_int32, P, P, P, P, P, P, N, c_int32, P, P, P]),
        'ptmi_adam_flat': (c_int32, [P, P, P, P, c_int32, c_int64, P, c_float, P, P, P, P, c_double, c_double, c_double, c_double,
                                     c_double, P, c_int32, P]),
        'ptmi_gl_partials_elems': (c_int64, []),
        'ptmi_pit_pairwise_sse': (c_int, [P, P, P, P, c_int64, c_int64, P, c_int32, c_int32, P, P, P, P]),     # HOST int64_t* strides
    }
    for name, (res, args) in pinned.items():
        got_res, got_args = _lib.SIGNATURES[name]
        assert got_res is res, (name, got_res)
        assert len(got_args) == len(args) and all(a is b for a, b in zip(got_args, args)), (name, got_args)
    assert _lib.StftGeom._fields_ == [('size', c_int32), ('shift', c_int32), ('window_length', c_int32), ('pad_left', c_int32),
                                      ('pad_right', c_int32), ('pad', c_int32)]
    assert _lib.NormGeom._fields_ == [('rank', c_int32), ('size', c_int64 * 5), ('stat_group_stride', c_int64 * 5),
                                      ('indep_stride', c_int64 * 5), ('batch_dim', c_int32), ('seq_dim', c_int32)]
    assert sizeof(_lib.StftGeom) == 24 and sizeof(_lib.NormGeom) == 136       # 4 + 4 padding + 3 * 40 + 2 * 4
    g = _lib.StftGeom(512, 128, 400, 1, 2, 3)
    assert (g.size, g.shift, g.window_length, g.pad_left, g.pad_right, g.pad) == (512, 128, 400, 1, 2, 3)


SYNTHETIC_HEADER = '''
#ifndef T_H_
#define T_H_
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif
#define PTMI_E_INVALID (-1)   /* ptmi_in_a_define_comment( */
#define PTMI_WRAP(x) \\
    ptmi_macro(x)
typedef void* ptmi_stream_t;
typedef struct ptmi_opaque ptmi_opaque;
typedef struct ptmi_box {
    int32_t a;          /* first */
    int32_t b, c;
    int64_t d[3];
} ptmi_box;
/* ptmi_foo( is only spoken of here;
 * int ptmi_in_a_comment(int x); */
const char* ptmi_name(void);
// int ptmi_line_comment(int x);
int64_t ptmi_count(const ptmi_box* g, int64_t n);
int
ptmi_launch(const float* x, const uint16_t* const* planes, ptmi_opaque** handle,
            const int64_t* strides, float taps[4], int32_t n, double lr, float eps,
            int code, ptmi_stream_t stream);
#ifdef __cplusplus
}
#endif
#endif
'''


def test_header_parser_on_a_synthetic_header():
    import ctypes
    from ctypes import POINTER, c_char_p, c_double, c_float, c_int, c_int32, c_int64, c_void_p
    from padertorch_amd import _capi

    class Box(ctypes.Structure):
        _fields_ = _capi.struct_fields(SYNTHETIC_HEADER, 'ptmi_box')
    assert Box._fields_ == [('a', c_int32), ('b', c_int32), ('c', c_int32), ('d', c_int64 * 3)]
    sigs = _capi.signatures(SYNTHETIC_HEADER, {'ptmi_box': Box})
    assert list(sigs) == ['ptmi_name', 'ptmi_count', 'ptmi_launch']            # nothing from comments or #define lines
    assert sigs['ptmi_name'] == (c_char_p, [])
    assert sigs['ptmi_count'] == (c_int64, [POINTER(Box), c_int64])
    assert sigs['ptmi_launch'] == (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int32, c_double, c_float, c_int, c_void_p])

    def rejected(declaration, name):
        with pytest.raises(ValueError, match=name):
            _capi.signatures(SYNTHETIC_HEADER.replace('const char* ptmi_name(void);', declaration), {'ptmi_box': Box})
    rejected('int ptmi_bad_scalar(unsigned int n);', 'ptmi_bad_scalar')             # not "type name"
    rejected('int ptmi_bad_type(size_t n);', 'ptmi_bad_type')                       # an unknown scalar type
    rejected('uint8_t ptmi_bad_return(int32_t n);', 'ptmi_bad_return')              # an unknown return type
    rejected('int ptmi_by_value(ptmi_box g);', 'ptmi_by_value')                     # a structure passed by value
    rejected('int ptmi_callback(void (*done)(int), int32_t n);', 'ptmi_callback')   # a function-pointer parameter
    rejected('int ptmi_unnamed(int32_t);', 'ptmi_unnamed')                          # a parameter without a name
    rejected('int ptmi_no_parens int32_t n;', 'ptmi_no_parens')                     # a declaration that cannot be split
    rejected('static const int ptmi_table = 3;', 'ptmi_table')                      # not a prototype at all
    rejected('int64_t ptmi_count(int32_t n);', 'ptmi_count')                        # declared twice
    # only the extern "C" bracket itself is taken out: what else stands between #ifdef __cplusplus and #endif is read like the rest
    rejected('#ifdef __cplusplus\nint ptmi_cxx_only(size_t n);\n#endif', 'ptmi_cxx_only')
    inside = _capi.signatures(SYNTHETIC_HEADER.replace('const char* ptmi_name(void);', '#ifdef __cplusplus\nint ptmi_cxx_only(int32_t n);\n#endif'),
                              {'ptmi_box': Box})
    assert inside['ptmi_cxx_only'] == (c_int, [c_int32])
    with pytest.raises(ValueError, match='extern "C"'):
        _capi.signatures(SYNTHETIC_HEADER.replace('}\n#endif\n#endif', '#endif\n#endif'), {'ptmi_box': Box})
    with pytest.raises(ValueError, match='ptmi_box'):
        _capi.struct_fields(SYNTHETIC_HEADER.replace('int64_t d[3];', 'float* d;'), 'ptmi_box')
    with pytest.raises(ValueError, match='ptmi_missing'):
        _capi.struct_fields(SYNTHETIC_HEADER, 'ptmi_missing')


def test_call_checks_under_the_symbols_own_name():
    """``_lib.call``: a refused launch raises ``'<symbol>: <message> (code <rc>)'``, a code the caller accepts comes back instead, and a
    name the header does not declare is an error (null arguments: the entry point refuses before anything touches a device)."""
    from padertorch_amd import _lib
    from padertorch_amd.build import build
    build()
    with pytest.raises(RuntimeError, match=r'^ptmi_gl_project: .+ \(code -1\)$'):
        _lib.call('ptmi_gl_project', None, None, 4, None, None)
    with pytest.raises(RuntimeError, match=r'^ptmi_gl_project: .+ \(code -1\)$'):
        _lib.call('ptmi_gl_project', None, None, 4, None, None, accept=(-2,))
    assert _lib.call('ptmi_gl_project', None, None, 4, None, None, accept=(-1,)) == -1
    with pytest.raises(AttributeError):
        _lib.call('ptmi_not_in_the_library')


def test_call_launches_timed_sites_through_timed(monkeypatch):
    """A launch with a ``timer`` goes through ``_lib.timed`` whether or not ``KERNEL_TIMERS`` is on - tools replace ``_lib.timed`` to take
    events of their own in exactly the steps that carry none (``scripts/phase_events.py``) - and one without a timer never does."""
    from padertorch_amd import _lib
    from padertorch_amd.build import build
    build()
    seen = []

    def timed(name, fn, *args):
        seen.append((name, fn, args, _lib.KERNEL_TIMERS))
        return fn(*args)
    monkeypatch.setattr(_lib, 'timed', timed)
    monkeypatch.setattr(_lib, 'KERNEL_TIMERS', None)
    args = (None, None, 4, None, None)
    assert _lib.call('ptmi_gl_project', *args, timer='gl_project', accept=(-1,)) == -1
    assert seen == [('gl_project', _lib.load().ptmi_gl_project, args, None)]
    with pytest.raises(RuntimeError, match=r'^ptmi_gl_project: .+ \(code -1\)$'):          # the code is checked behind the bracket
        _lib.call('ptmi_gl_project', *args, timer='gl_project')
    assert len(seen) == 2
    for untimed in (None, ''):                                                              # ('': stft_forward's "not timed")
        assert _lib.call('ptmi_gl_project', *args, timer=untimed, accept=(-1,)) == -1
    assert _lib.call('ptmi_gl_project', *args, accept=(-1,)) == -1
    assert len(seen) == 2
