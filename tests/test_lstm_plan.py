"""The geometry queries of the persistent LSTM recurrence answer what they answered before they moved onto one plan per direction
(csrc/lstm.hip: fwd_plan / bwd_plan).  Host functions only: no GPU needed.

The answers depend on the CU count of the current device.  Without a device the library assumes 256, and an MI355X has 256, so the
one recorded table (tests/golden/g19_lstm_plan.json, made by tests/golden/make_golden_lstm_plan.py from the library of the commit
before the move) holds on a build machine and on the GPU machine alike."""
import importlib.util
import json
from pathlib import Path

GOLDEN = Path(__file__).resolve().parent / 'golden'


def _maker():
    spec = importlib.util.spec_from_file_location('make_golden_lstm_plan', GOLDEN / 'make_golden_lstm_plan.py')
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_plan_queries_answer_as_recorded():
    from padertorch_amd import _lib
    from padertorch_amd.build import build
    build()
    maker = _maker()
    rec = json.loads((GOLDEN / 'g19_lstm_plan.json').read_text())
    assert rec['grid'] == maker.GRID == {
        'H': [4, 6, 8, 36, 100, 600, 640, 644, 768, 772, 1024], 'max_batch': [1, 16, 17, 32, 33, 64, 65, 96, 112, 256],
        'ndir': [1, 2], 'T': [1, 253]}
    got = maker.table(maker.load(_lib.LIB_PATH))
    assert set(got) == set(rec['answers'])
    for name, want in rec['answers'].items():
        assert len(want) > 0 and got[name] == want, (name, [i for i, (a, b) in enumerate(zip(got[name], want)) if a != b][:10])
    # the table is not trivial: every query has both kinds of answer in it
    for name in ('handoff_cols', 'forward_fills', 'backward_planes_ok'):
        assert 0 in rec['answers'][name] and any(rec['answers'][name]), name


def test_multi_launch_shape_is_past_the_one_launch_limit():
    """tests/test_gpu_lstm.py runs H = 600, max_batch = 112, ndir = 2 as the shape whose forward AND backward recurrence take two
    launches on 256 CUs.  The plans for it: forward 32-row x 12-unit tiles, 50 workgroups per chain, 4 row tiles, 2 per launch (100
    workgroups per row tile, 256 CUs); backward 32-row tiles, 38 workgroups per chain, 4 row tiles, 3 per launch (76 per row tile,
    240 resident).  What the C ABI shows of that: a forward call fills the backward planes only when it is ONE launch - a batch of
    64 (2 row tiles) is, 112 is not, while the persistent kernels still run it (its planes are GEMM operands)."""
    maker = _maker()
    from padertorch_amd import _lib
    lib = maker.load(_lib.LIB_PATH)
    assert lib.ptmi_lstm_handoff_cols(600, 0) == 608 and lib.ptmi_lstm_handoff_cols(600, 1) == 2400
    assert lib.ptmi_lstm_forward_fills(4, 2, 64, 600) == 2
    assert lib.ptmi_lstm_forward_fills(4, 2, 112, 600) == 0
    assert lib.ptmi_lstm_backward_planes_ok(4, 2, 112, 4 * 112, 600) == 1
