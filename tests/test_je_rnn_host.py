"""contrib/je's RNN wrappers and poolings without a GPU: the fp64 restatement (tests/je_rnn_ref.py) against the reference's own fp64 run
(tests/golden/g25_je_rnn.npz), constructors, state_dict and config behaviour, the refusals, the stride arithmetic of ``seq_pool`` and the
registration of the kernels."""
import importlib.util
import json
import re
from pathlib import Path

import numpy as np
import pytest
import torch

import je_rnn_ref as ref

REPO = Path(__file__).resolve().parent.parent
GOLDEN = REPO / 'tests' / 'golden'
OPS = ('chunk_gru_forward', 'chunk_gru_backward', 'seq_table', 'seq_gather', 'seq_pool_forward', 'seq_pool_backward')
EXACT = 1e-11            # fp64 against fp64: relative to max|want|
MODES = {'Sum': 'sum', 'Mean': 'mean', 'Max': 'max', 'TakeLast': 'last'}


@pytest.fixture(scope='module')
def g25():
    d = dict(np.load(GOLDEN / 'g25_je_rnn.npz', allow_pickle=False))
    spec = importlib.util.spec_from_file_location('make_golden_je_rnn', GOLDEN / 'make_golden_je_rnn.py')
    d['maker'] = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(d['maker'])             # for the seeded inputs (the reference is not imported)
    return d


def same(name, got, want):
    got, want = got.detach().double().reshape(-1), torch.as_tensor(want).double().reshape(-1)
    assert got.shape == want.shape, (name, got.shape, want.shape)
    scale = max(float(want.abs().max()), 1e-300)
    assert float((got - want).abs().max()) <= EXACT * scale, (name, float((got - want).abs().max()), scale)


def test_fixture_is_what_its_generator_describes(g25):
    mk = g25['maker']
    assert json.loads(str(g25['rnn_cases'])) == {k: list(v) for k, v in mk.RNN_CASES.items()}
    assert g25['lengths'].tolist() == mk.LENGTHS == sorted(mk.LENGTHS, reverse=True)
    assert (GOLDEN / 'g25_je_rnn.npz').stat().st_size < 1 << 20
    for case in mk.RNN_CASES:
        x, r = mk.rnn_inputs(case)
        assert g25[case + '_y64'].shape == r.shape and g25[case + '_g64_x'].shape == x.shape


@pytest.mark.parametrize('case', ['r0', 'r1', 'r4'])
def test_gru_restatement_matches_the_reference(g25, case):
    mk = g25['maker']
    kind, H, layers, bidir, bias, reverse, lengths = mk.RNN_CASES[case]
    state = {k: g25[f'{case}_p_{k}'] for k in json.loads(str(g25[case + '_keys']))}
    names = json.loads(str(g25[case + '_names']))
    stack = ref.gru_layers_from_state(state, 'rnn.rnn.', layers, bidir, bias)
    params = {}
    for k, dirs in enumerate(stack):
        for d, suffix in enumerate(('', '_reverse')[:len(dirs)]):
            for t, n in zip(dirs[d], ('weight_ih', 'weight_hh', 'bias_ih', 'bias_hh')):
                if t is not None:
                    params[f'rnn.rnn.{n}_l{k}{suffix}'] = t.requires_grad_()
    x0, r0 = mk.rnn_inputs(case)
    x = torch.from_numpy(x0).double().requires_grad_()
    y = ref.gru_stack(x, lengths, stack, reverse)
    if kind == 'gru+autopool':
        params['pool.alpha'] = torch.from_numpy(state['pool.alpha']).double().requires_grad_()
        y = ref.seq_pool(y, lengths, -1, 'autopool', alpha=params['pool.alpha'])
    same('y', y, g25[case + '_y64'])
    assert sorted(params) == sorted(names)
    grads = torch.autograd.grad((y * torch.from_numpy(r0).double()).sum(), [x] + [params[n] for n in names])
    same('dx', grads[0], g25[case + '_g64_x'])
    for n, g in zip(names, grads[1:]):
        same(n, g, g25[f'{case}_g64_{n}'])


def test_pooling_restatement_matches_the_reference(g25):
    mk = g25['maker']
    for key, name, wl, axis, keep in mk.pool_cases():
        x = torch.from_numpy(mk.pool_inputs(key)).double().requires_grad_()
        out = ref.seq_pool(x, mk.LENGTHS if wl else None, axis, MODES[name], keep)
        if name == 'Max':
            assert torch.equal(out[1], torch.from_numpy(g25[key + '_idx'])), key
            out = out[0]
        assert tuple(out.shape) == g25[key + '_y64'].shape, key
        same(key, out, g25[key + '_y64'])
        _, r = mk.pool_inputs(key, tuple(out.shape))
        same(key + ' dx', torch.autograd.grad((out * torch.from_numpy(r).double()).sum(), x)[0], g25[key + '_g64_x'])


def test_autopool_and_reverse_restatements_match_the_reference(g25):
    mk = g25['maker']
    for trainable in 'tf':
        for wl in 'ln':
            key = f'a_{trainable}_{wl}'
            x = torch.from_numpy(mk.pool_inputs(key)).double().requires_grad_()
            alpha = torch.full((mk.F, 1), mk.ALPHA, dtype=torch.float64, requires_grad=True)
            out = ref.seq_pool(x, mk.LENGTHS if wl == 'l' else None, -1, 'autopool', alpha=alpha if trainable == 't' else mk.ALPHA)
            same(key, out, g25[key + '_y64'])
            _, r = mk.pool_inputs(key, tuple(out.shape))
            grads = torch.autograd.grad((out * torch.from_numpy(r).double()).sum(), [x] + ([alpha] if trainable == 't' else []))
            same(key + ' dx', grads[0], g25[key + '_g64_x'])
            if trainable == 't':
                same(key + ' dalpha', grads[1], g25[key + '_g64_alpha'])
    for wl in 'ln':
        key = f'v_{wl}'
        x = torch.from_numpy(mk.pool_inputs(key)).double().requires_grad_()
        out = ref.reverse_sequence(x, mk.LENGTHS if wl == 'l' else None)
        same(key, out, g25[key + '_y64'])
        _, r = mk.pool_inputs(key, tuple(out.shape))
        same(key + ' dx', torch.autograd.grad((out * torch.from_numpy(r).double()).sum(), x)[0], g25[key + '_g64_x'])
    nan = torch.full((1, 4, 2), 1., dtype=torch.float64)
    nan[0, 3] = float('nan')
    out = ref.reverse_sequence(nan, [2])                # behind the length: x[(2 - 1 - t) mod 4] * 0 -> t = 2 reads position 3: NaN stays
    assert torch.isnan(out[0, 2]).all() and (out[0, 3] == 0).all() and (out[0, :2] == 1).all()


def test_length_arithmetic():
    assert ref.mean_denominator(3) == float(np.float32(3.) + np.float32(1e-6)) == 3.0000009536743164
    assert ref.mean_denominator(0) == float(np.float32(1e-6))
    x = torch.arange(24, dtype=torch.float64).reshape(2, 3, 4)
    assert ref.seq_pool(x, [0, 2], -1, 'sum').tolist() == [[0., 0., 0.], [25., 33., 41.]]
    assert ref.seq_pool(x, [0, 2], -1, 'mean')[0].tolist() == [0., 0., 0.]
    v, i = ref.seq_pool(x, [0, 9], -1, 'max')
    assert v[0].tolist() == [-np.inf] * 3 and i[0].tolist() == [0, 0, 0] and i[1].tolist() == [3, 3, 3]      # lengths are clipped to T
    assert ref.seq_pool(x, [1, 4], 2, 'last', keepdims=True).shape == (2, 3, 1)
    assert ref.seq_pool(x, [1, 3], 1, 'last').tolist() == [[0., 1., 2., 3.], [20., 21., 22., 23.]]


def test_stride_collapse():
    from padertorch_amd.ops.seq_pool import _collapse, geometry
    assert _collapse((), ()) == (1, 0) and _collapse((3, 4), (4, 1)) == (12, 1) and _collapse((3, 4), (8, 1)) is None
    assert _collapse((1, 4), (77, 2)) == (4, 2)
    x = torch.zeros(2, 5, 7)
    assert geometry(x, 2)[1:] == ([2, 5, 7, 1], [35, 7, 1, 0])
    assert geometry(x, 1)[1:] == ([2, 1, 5, 7], [35, 0, 7, 1])
    y = x.transpose(1, 2)                               # [2, 7, 5]: the RNN's output view, time strided
    g = geometry(y, 2)
    assert g[0] is y and g[1:] == ([2, 7, 5, 1], [35, 1, 7, 0])
    z = torch.zeros(2, 3, 4, 6)[:, :, ::3]              # [2, 3, 2, 6], strides (72, 24, 18, 1): (C, F) do not collapse -> one copy
    g = geometry(z, 3)
    assert g[0] is not z and g[0].is_contiguous() and g[1:] == ([2, 6, 6, 1], [36, 6, 1, 0])
    assert geometry(torch.zeros(2, 3, 4, 6), 3)[1:] == ([2, 12, 6, 1], [72, 6, 1, 0])


def test_constructors_state_dict_and_configs(g25):
    from padertorch_amd.contrib.je import modules as je
    from padertorch_amd.contrib.je.modules import reduce, rnn
    mk = g25['maker']
    assert {'RNN', 'GRU', 'LSTM', 'TransformerEncoder', 'reverse_sequence', 'Sum', 'Mean', 'Max', 'TakeLast', 'AutoPool'} <= set(dir(je))
    for case, (kind, H, layers, bidir, bias, reverse, _) in mk.RNN_CASES.items():
        if kind == 'transformer':
            net = rnn.TransformerEncoder(je.TransformerLayerStack(mk.F, H, num_layers=layers, **mk.TRANSFORMER), reverse=reverse)
        else:
            cls = torch.nn.LSTM if kind == 'lstm' else torch.nn.GRU
            net = (rnn.LSTM if kind == 'lstm' else rnn.GRU)(cls(mk.F, H, layers, bias=bias, batch_first=True, bidirectional=bidir), reverse=reverse)
        keys = [k for k in json.loads(str(g25[case + '_keys'])) if k.startswith('rnn.')]
        assert ['rnn.' + k for k in net.state_dict()] == keys
        net.load_state_dict({k[4:]: torch.from_numpy(g25[f'{case}_p_{k}']) for k in keys}, strict=True)
        assert ['rnn.' + n for n, _ in net.named_parameters()] == [n for n in json.loads(str(g25[case + '_names'])) if n.startswith('rnn.')]
        assert net.reverse is reverse and net.output_net is None
    pool = reduce.AutoPool(12, alpha=1.5, trainable=True)
    assert list(pool.state_dict()) == ['alpha'] and tuple(pool.alpha.shape) == (12, 1) and float(pool.alpha.detach()[3]) == 1.5
    assert reduce.AutoPool(12).alpha == 1. and not list(reduce.AutoPool(12).parameters())
    for cls in (reduce.Sum, reduce.Mean, reduce.Max, reduce.TakeLast):
        m = cls()
        assert (m.axis, m.keepdims) == (-1, False) and (cls(axis=1, keepdims=True).axis, cls(1, True).keepdims) == (1, True)
    config = dict(rnn=None, output_net=None)
    rnn.GRU.finalize_dogmatic_config(config)
    assert config['rnn'] == dict(factory=torch.nn.GRU, num_layers=1, bias=True, dropout=0., bidirectional=False, batch_first=True)
    rnn.LSTM.finalize_dogmatic_config(config)
    assert config['rnn']['factory'] is torch.nn.LSTM and config['rnn']['batch_first'] is True
    rnn.TransformerEncoder.finalize_dogmatic_config(config)
    assert config['rnn'] == dict(factory=je.TransformerLayerStack, num_layers=6, hidden_size=512, num_heads=8, d_ff=2048, bidirectional=False,
                                 cross_attention=False, activation_ff='relu', dropout=0., positional_encoding=True)
    with pytest.raises(NotImplementedError, match='CNN1d'):
        rnn.GRU.finalize_dogmatic_config(dict(rnn=None, output_net=dict(out_channels=[8])))
    net = rnn.GRU(torch.nn.GRU(4, 3, 2, batch_first=True))
    net.freeze(1)
    assert [p.requires_grad for _, p in net.rnn.named_parameters()] == [False] * 4 + [True] * 4
    assert rnn.RNN(None)('x', 'l') == ('x', 'l')         # no rnn, no output_net: the identity


def test_refusals():
    from padertorch_amd.contrib.je.modules import reduce, rnn
    from padertorch_amd.ops import gru, seq_pool
    with pytest.raises(NotImplementedError, match='no HIP kernel'):
        rnn.RNN(torch.nn.RNN(4, 3, batch_first=True))
    with pytest.raises(NotImplementedError, match='proj_size'):
        rnn.LSTM(torch.nn.LSTM(4, 6, proj_size=3, batch_first=True))
    with pytest.raises(NotImplementedError, match='without biases'):
        rnn.LSTM(torch.nn.LSTM(4, 6, bias=False, batch_first=True))
    rnn.GRU(torch.nn.GRU(4, 129, batch_first=True))                      # above 128 units W_hh is streamed, not refused
    with pytest.raises(NotImplementedError, match='bound of 1792'):
        rnn.GRU(torch.nn.GRU(4, 1793, batch_first=True))
    with pytest.raises(NotImplementedError, match='bound of 1536'):
        rnn.LSTM(torch.nn.LSTM(4, 1537, batch_first=True))
    x = torch.zeros(2, 4, 5)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        rnn.GRU(torch.nn.GRU(4, 3, batch_first=True))(x, [5, 2])
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        rnn.LSTM(torch.nn.LSTM(4, 3, batch_first=True), reverse=True)(x, None)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        rnn.reverse_sequence(x, [4, 2])
    for m in (reduce.Sum(), reduce.Mean(axis=1), reduce.Max(), reduce.TakeLast(), reduce.AutoPool(4), reduce.AutoPool(4, trainable=True)):
        with pytest.raises(RuntimeError, match='no CPU fallback'):
            m(x, [5, 2])
    with pytest.raises(NotImplementedError, match='float32 only'):
        reduce.Sum()(x.double())
    with pytest.raises(NotImplementedError, match='float32 only'):
        rnn.reverse_sequence(x.half())
    with pytest.raises(ValueError, match='axis >= 1'):
        seq_pool.seq_pool(x, None, 0, 'sum')
    with pytest.raises(ValueError, match='mode one of'):
        seq_pool.seq_pool(x, None, 1, 'median')
    w = torch.zeros(9, 4)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        gru.chunk_gru(torch.zeros(6, 4), torch.zeros(1, 3, dtype=torch.int32), 6, w, torch.zeros(9, 3))
    with pytest.raises(NotImplementedError, match='float32 only'):
        gru.chunk_gru(torch.zeros(6, 4, dtype=torch.float64), torch.zeros(1, 3, dtype=torch.int32), 6, w, torch.zeros(9, 3))


def test_ops_have_a_cuda_kernel_only():
    import padertorch_amd  # noqa: F401
    from padertorch_amd import ops
    assert ops.chunk_gru is ops.gru.chunk_gru and ops.reverse_sequence is ops.seq_pool.reverse_sequence
    for n in OPS:
        assert getattr(torch.ops.ptmi, n).default._schema.name == f'ptmi::{n}'
        assert torch._C._dispatch_has_kernel_for_dispatch_key(f'ptmi::{n}', 'CUDA')
        assert not torch._C._dispatch_has_kernel_for_dispatch_key(f'ptmi::{n}', 'CPU')


def test_header_library_and_bounds_agree():
    import ctypes
    from padertorch_amd import _lib
    from padertorch_amd.build import build
    from padertorch_amd.ops import gru
    text = re.sub(r'/\*.*?\*/', '', (REPO / 'include' / 'ptmi.h').read_text(), flags=re.S)
    names = set(re.findall(r'\b(ptmi_(?:chunk_gru|seq)_[a-z0-9_]+)\s*\(', text))
    assert len(names) == 9 and names == {n for n in _lib.SIGNATURES if n.startswith(('ptmi_chunk_gru_', 'ptmi_seq_'))}
    build()
    lib = ctypes.CDLL(str(_lib.LIB_PATH))
    for n in names:
        assert hasattr(lib, n), n
    lib = _lib.load()
    # the streamed backward kernel keeps 5 words per (sequence of the tile, unit) in LDS; a CU has 160 KB
    H, tile = lib.ptmi_chunk_gru_max_hidden(), lib.ptmi_chunk_gru_tile()
    assert (H, tile, lib.ptmi_chunk_gru_max_resident_hidden()) == (1792, 4, 128) == (gru.MAX_HIDDEN, 4, gru.RESIDENT_HIDDEN)
    assert 5 * tile * H * 4 + 64 <= 160 * 1024 < 5 * tile * 2049 * 4
