"""The planes GEMM's plan and workspace queries answer what they answered before the host half of csrc/gemm_planes.hip moved onto one
planner (``plan_call``) and one launch path.  Host functions only: no GPU needed.

The answers depend on the CU count of the current device.  Without a device the library assumes 256, and an MI355X has 256, so the
one recorded table (tests/golden/g20_gemm_plan.json, made by tests/golden/make_golden_gemm_plan.py from the library of the commit
before the move) holds on a build machine and on the GPU machine alike."""
import importlib.util
import json
from pathlib import Path

GOLDEN = Path(__file__).resolve().parent / 'golden'


def _maker():
    spec = importlib.util.spec_from_file_location('make_golden_gemm_plan', GOLDEN / 'make_golden_gemm_plan.py')
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _lib_and_maker():
    from padertorch_amd import _lib
    from padertorch_amd.build import build
    build()
    maker = _maker()
    return maker.load(_lib.LIB_PATH), maker


def test_plan_queries_answer_as_recorded():
    lib, maker = _lib_and_maker()
    rec = json.loads((GOLDEN / 'g20_gemm_plan.json').read_text())
    assert rec['grid'] == maker.GRID
    grid = rec['grid']
    # the grid brackets every rule (see the maker's docstring)
    assert grid['split_k'] == [1, 2, 3, 8, 12, -1, -4]
    for name in ('M', 'N'):
        assert {1, 16, 32192, 70000} <= set(grid[name])
    assert {1, 31, 33, 127, 128, 8096, 32192, 40000} <= set(grid['K'])
    assert {len(ns) for ns, _ in grid['group_blocks']} == {1, 2, 3}
    assert any(len(blocks) < 2 * len(ns) for ns, blocks in grid['group_blocks'])                # skipped blocks
    assert {m_split % 16 == 0 for _, m_split in grid['group_m']} == {True, False}
    got = maker.table(lib)
    assert set(got) == set(rec['answers'])
    for name, want in rec['answers'].items():
        assert len(want) > 0 and got[name] == want, (name, [(i, a, b) for i, (a, b) in enumerate(zip(got[name], want)) if a != b][:10])
    # the table is not trivial: every tile index and more than one k-range count occur, with no tile pinned as well as with one
    for name in ('plan', 'pinned_plan', 'group_plan'):
        assert {v // 100 for v in rec['answers'][name]} == set(range(6)), name
        assert len({v % 100 for v in rec['answers'][name]}) > 1, name
    assert min(rec['answers']['workspace_elems']) == 0 < max(rec['answers']['workspace_elems'])


def test_known_plans():
    """What the planner answered before the move for the shapes the training step and the tile tests meet, as literals (256 CUs, no
    tile pinned): 100 * tile + k ranges, tile 5 = the 128 x 128 kernel / a grouped call that is refused."""
    lib, maker = _lib_and_maker()
    with maker.pinned(None):
        assert lib.ptmi_gemm_planes_plan(2400, 1200, 8096, 12) == 105             # 256 x 256 tiles, 5 of the 12 ranges allowed
        assert lib.ptmi_gemm_planes_plan(8096, 4800, 257, 1) == 1
        assert lib.ptmi_gemm_planes_plan(4800, 1200, 1000, -1) == 501             # negative: the 128 x 128 kernel as asked for
        assert lib.ptmi_gemm_planes_plan(70000, 4800, 40000, 1) == 501            # planes of 2 GB and more
        assert lib.ptmi_gemm_planes_plan(0, 5, 5, 1) == -1
        lstm_blocks = [0, 1, 3, 5]                                                # {dG_f, dG_b} x {X, H_f, H_b} without (f, H_b), (b, H_f)
        assert lib.ptmi_gemm_planes_group_plan(*maker.group_args(4800, 2400, [257, 600, 600], lstm_blocks, 8096, 12)) == 4
        assert lib.ptmi_gemm_planes_group_plan(*maker.group_args(4800, 2408, [257, 600, 600], lstm_blocks, 8096, 12)) == 504
        assert lib.ptmi_gemm_planes_group_plan(*maker.group_args(4800, 4800, [257], [0], 8096, 12)) == -1
        assert lib.ptmi_gemm_planes_group_workspace_elems(*maker.group_args(4800, 2400, [257], [], 8096, 12)) == 0
