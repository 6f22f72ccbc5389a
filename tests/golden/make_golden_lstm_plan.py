"""Record what the persistent LSTM recurrence's geometry queries answer: tests/golden/g19_lstm_plan.json.

    PTMI_LIB=/path/to/libptmi.so python tests/golden/make_golden_lstm_plan.py        # default: padertorch_amd/libptmi.so

The queries are pure host functions of (T, ndir, max_batch, rows, H) and the CU count of the current device (256 without a device).
The file was recorded from the library of the commit BEFORE the queries moved onto fwd_plan / bwd_plan (csrc/lstm.hip); the grid
brackets every threshold of those rules.  tests/test_lstm_plan.py walks the same grid (``table`` below) and demands equality."""
import ctypes
import json
import os
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent.parent
OUT = Path(__file__).resolve().parent / 'g19_lstm_plan.json'

GRID = {
    'H': [4, 6, 8, 36, 100, 600, 640, 644, 768, 772, 1024],
    'max_batch': [1, 16, 17, 32, 33, 64, 65, 96, 112, 256],
    'ndir': [1, 2],
    'T': [1, 253],
}


def load(path=None):
    lib = ctypes.CDLL(str(path or os.environ.get('PTMI_LIB') or ROOT / 'padertorch_amd' / 'libptmi.so'))
    i32, i64 = ctypes.c_int32, ctypes.c_int64
    for name, res, args in (('ptmi_lstm_handoff_cols', i32, [i32, i32]), ('ptmi_lstm_forward_fills', ctypes.c_int, [i32] * 4),
                            ('ptmi_lstm_backward_planes_ok', i32, [i32, i32, i32, i64, i32]),
                            ('ptmi_lstm_scratch_elems', i64, [i32] * 5), ('ptmi_lstm_flags_elems', i64, [i32] * 3)):
        getattr(lib, name).restype, getattr(lib, name).argtypes = res, args
    return lib


def table(lib):
    """Every query over GRID, loops nested in the order H, max_batch, ndir, T (rows: equal, then unequal to T * max_batch)."""
    out = {'handoff_cols': [], 'forward_fills': [], 'backward_planes_ok': [], 'scratch_elems': [], 'flags_elems': []}
    for H in GRID['H']:
        out['handoff_cols'] += [lib.ptmi_lstm_handoff_cols(H, 0), lib.ptmi_lstm_handoff_cols(H, 1)]
        for B in GRID['max_batch']:
            for ndir in GRID['ndir']:
                for T in GRID['T']:
                    out['forward_fills'].append(lib.ptmi_lstm_forward_fills(T, ndir, B, H))
                    out['backward_planes_ok'] += [lib.ptmi_lstm_backward_planes_ok(T, ndir, B, T * B, H),
                                                  lib.ptmi_lstm_backward_planes_ok(T, ndir, B, T * B - 1, H)]
                    out['scratch_elems'] += [lib.ptmi_lstm_scratch_elems(T, ndir, B, H, 0), lib.ptmi_lstm_scratch_elems(T, ndir, B, H, 1)]
    for B in GRID['max_batch']:
        for ndir in GRID['ndir']:
            for T in GRID['T']:
                out['flags_elems'].append(lib.ptmi_lstm_flags_elems(T, ndir, B))
    return out


if __name__ == '__main__':
    OUT.write_text(json.dumps({'grid': GRID, 'answers': table(load())}, separators=(',', ':')) + '\n')
    print(OUT, OUT.stat().st_size, 'bytes')
