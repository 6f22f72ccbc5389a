"""Record what the planes GEMM's plan and workspace queries answer: tests/golden/g20_gemm_plan.json.

    PTMI_LIB=/path/to/libptmi.so python tests/golden/make_golden_gemm_plan.py        # default: padertorch_amd/libptmi.so

The queries are pure host functions of the shapes, ``split_k``, ``PTMI_GEMM_TILE`` and the CU count of the current device (256 without
a device).  The file was recorded from the library of the commit BEFORE the host half of csrc/gemm_planes.hip moved onto one planner
(``plan_call``); the grid brackets every rule of it: the clamp of ``split_k`` to whole k blocks, the ``KB / 4`` cap of the cost model,
negative ``split_k`` (exactly that many ranges on the 128 x 128 kernel), a pinned tile, planes of 2 GB and more, and for the grouped
call skipped blocks and an ``m_split`` that is no multiple of 16.  tests/test_gemm_plan.py walks the same grid (``table`` below) and
demands equality."""
import ctypes
import json
import os
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent.parent
OUT = Path(__file__).resolve().parent / 'g20_gemm_plan.json'

SPLITS = [1, 2, 3, 8, 12, -1, -4]
GRID = {
    'split_k': SPLITS,
    # plain calls, no tile pinned: plan over M x N x K x split_k; workspace over ws_M x ws_N x K x split_k
    'M': [1, 16, 257, 1200, 2400, 4800, 32192, 70000],
    'N': [1, 16, 600, 1200, 4800, 32192, 70000],
    'K': [1, 31, 33, 127, 128, 129, 257, 1000, 8096, 32192, 40000],
    'ws_M': [1, 257, 70000],
    'ws_N': [16, 4800],
    # plain calls with PTMI_GEMM_TILE = 0..5
    'pinned_M': [16, 2400, 70000],
    'pinned_N': [1200, 4800],
    'pinned_K': [33, 1000, 8096, 40000],
    # grouped calls: (m, m_split) x (segment widths, blocks that are there: part * segments + segment) x K x split_k
    'group_m': [[4800, 2400], [4800, 2408], [70000, 35008]],
    'group_blocks': [[[600], [0, 1]], [[600], [1]], [[257, 600], [0, 1, 2, 3]], [[257, 600], [0, 3]],
                     [[257, 600, 600], [0, 1, 2, 3, 4, 5]], [[257, 600, 600], [0, 1, 3, 5]],
                     [[1200, 1, 16], [0, 1, 2, 3, 4, 5]], [[1200, 1, 16], [2, 3]]],
    'group_K': [33, 257, 1000, 8096, 32192],
    # grouped calls with PTMI_GEMM_TILE = 0..5: group_m[0] x group_blocks[5] x pinned_group_K x split_k
    'pinned_group_K': [1000, 8096],
}


def load(path=None):
    lib = ctypes.CDLL(str(path or os.environ.get('PTMI_LIB') or ROOT / 'padertorch_amd' / 'libptmi.so'))
    i32, i64, ptr = ctypes.c_int32, ctypes.c_int64, ctypes.c_void_p
    for name, res, args in (('ptmi_gemm_planes_plan', i32, [i32] * 4), ('ptmi_gemm_planes_workspace_elems', i64, [i32] * 4),
                            ('ptmi_gemm_planes_group_plan', i32, [i32, i32, ptr, i32, ptr, i32, i32]),
                            ('ptmi_gemm_planes_group_workspace_elems', i64, [i32, i32, ptr, i32, ptr, i32, i32])):
        getattr(lib, name).restype, getattr(lib, name).argtypes = res, args
    return lib


def group_args(m, m_split, ns, blocks, k, split_k):
    """The argument list of the two grouped queries (of the output pointers only whether a block is there is read)."""
    c = (ctypes.c_void_p * (2 * len(ns)))()
    for blk in blocks:
        c[blk] = 1
    return m, m_split, (ctypes.c_int32 * len(ns))(*ns), len(ns), c, k, split_k


class pinned:
    """``with pinned(t):`` PTMI_GEMM_TILE = t (``None``: unset) - the library reads it at every call."""

    def __init__(self, tile):
        self.tile = tile

    def __enter__(self):
        self.before = os.environ.pop('PTMI_GEMM_TILE', None)
        if self.tile is not None:
            os.environ['PTMI_GEMM_TILE'] = str(self.tile)

    def __exit__(self, *exc):
        os.environ.pop('PTMI_GEMM_TILE', None)
        if self.before is not None:
            os.environ['PTMI_GEMM_TILE'] = self.before


def table(lib):
    """Every query over GRID, loops nested in the order the keys of GRID are listed in, ``split_k`` innermost, a pinned tile outermost."""
    out = {'plan': [], 'workspace_elems': [], 'pinned_plan': [], 'group_plan': [], 'group_workspace_elems': [], 'pinned_group_plan': []}
    with pinned(None):
        for M in GRID['M']:
            for N in GRID['N']:
                for K in GRID['K']:
                    out['plan'] += [lib.ptmi_gemm_planes_plan(M, N, K, s) for s in SPLITS]
        for M in GRID['ws_M']:
            for N in GRID['ws_N']:
                for K in GRID['K']:
                    out['workspace_elems'] += [lib.ptmi_gemm_planes_workspace_elems(M, N, K, s) for s in SPLITS]
        for m, m_split in GRID['group_m']:
            for ns, blocks in GRID['group_blocks']:
                for K in GRID['group_K']:
                    for s in SPLITS:
                        args = group_args(m, m_split, ns, blocks, K, s)
                        out['group_plan'].append(lib.ptmi_gemm_planes_group_plan(*args))
                        out['group_workspace_elems'].append(lib.ptmi_gemm_planes_group_workspace_elems(*args))
    for tile in range(6):
        with pinned(tile):
            for M in GRID['pinned_M']:
                for N in GRID['pinned_N']:
                    for K in GRID['pinned_K']:
                        out['pinned_plan'] += [lib.ptmi_gemm_planes_plan(M, N, K, s) for s in SPLITS]
            (m, m_split), (ns, blocks) = GRID['group_m'][0], GRID['group_blocks'][5]
            for K in GRID['pinned_group_K']:
                out['pinned_group_plan'] += [lib.ptmi_gemm_planes_group_plan(*group_args(m, m_split, ns, blocks, K, s)) for s in SPLITS]
    return out


if __name__ == '__main__':
    OUT.write_text(json.dumps({'grid': GRID, 'answers': table(load())}, separators=(',', ':')) + '\n')
    print(OUT, OUT.stat().st_size, 'bytes')
