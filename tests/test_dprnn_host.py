"""DPRNN without a GPU: constructor, state_dict layout against the reference's (tests/golden/g17_dprnn.npz), the chunk arithmetic, the
refusals and the registration of the kernels."""
import json
import re
from pathlib import Path

import numpy as np
import pytest
import torch

REPO = Path(__file__).resolve().parent.parent
GOLDEN = REPO / 'tests' / 'golden'
OPS = ('dprnn_tables', 'chunk_lstm_forward', 'chunk_lstm_backward', 'dprnn_colsum', 'dprnn_colsum_pair', 'dprnn_norm_residual_forward',
       'dprnn_norm_residual_backward', 'dprnn_segment', 'dprnn_overlap_add')


@pytest.fixture(scope='module')
def g17():
    d = dict(np.load(GOLDEN / 'g17_dprnn.npz', allow_pickle=False))
    d['cases'] = json.loads(str(d['cases']))
    return d


def test_constructor_defaults_and_attributes():
    from padertorch_amd.modules import DPRNN, DPRNNBlock, _ChunkRNN, overlap_add, segment  # noqa: F401
    net = DPRNN(64, 128, 100, 50, 6)
    assert (net.input_size, net.hidden_size, net.window_size, net.hop_size) == (64, 64, 100, 50)
    assert len(net.dprnn_blocks) == 6 and isinstance(net.dprnn_blocks[0], DPRNNBlock)
    chunk = net.dprnn_blocks[0].intra_chunk_rnn
    assert isinstance(chunk, _ChunkRNN) and chunk.lstm_reshape_to == '(b s) k n' and chunk.feat_size == 64
    assert net.dprnn_blocks[0].inter_chunk_rnn.lstm_reshape_to == '(b k) s n'
    assert isinstance(chunk.rnn, torch.nn.LSTM) and chunk.rnn.bidirectional and chunk.rnn.batch_first and chunk.rnn.hidden_size == 128
    assert chunk.fc.in_features == 256 and chunk.fc.out_features == 64 and tuple(chunk.norm.normalized_shape) == (64,)
    uni = DPRNNBlock(8, 5, inter_chunk_type='lstm')
    assert not uni.inter_chunk_rnn.rnn.bidirectional and uni.inter_chunk_rnn.fc.in_features == 5 and uni.intra_chunk_rnn.rnn.bidirectional
    assert net.flatten_parameters() is None and chunk.flatten_parameters() is None


@pytest.mark.parametrize('i', [0, 1, 2, 3])
def test_state_dict_matches_the_reference(g17, i):
    from padertorch_amd.modules import DPRNN
    N, H, K, P, blocks, intra, inter, _, _, _ = g17['cases'][i]
    net = DPRNN(N, H, K, P, blocks, inter_chunk_type=inter, intra_chunk_type=intra)
    keys = json.loads(str(g17[f'c{i}_keys']))
    state = net.state_dict()
    assert list(state) == keys
    assert [tuple(state[k].shape) for k in keys] == [g17[f'c{i}_p_{k}'].shape for k in keys]
    assert [n for n, _ in net.named_parameters()] == json.loads(str(g17[f'c{i}_names']))
    net.load_state_dict({k: torch.from_numpy(g17[f'c{i}_p_{k}']) for k in keys}, strict=True)


def test_chunk_arithmetic_matches_the_reference_doctests():
    from padertorch_amd.ops import dprnn
    # (L, hop, window, length) -> (S, S_b): dual_path_rnn.py:75-121
    for L, P, K, n, S, S_b in ((5, 2, 4, 5, 4, 4), (5, 2, 4, 4, 4, 3), (4, 2, 4, 4, 3, 3), (5, 2, 4, 3, 4, 3), (3, 2, 4, 3, 3, 3),
                               (5, 3, 4, 5, 2, 2), (5, 1, 4, 5, 8, 8), (7912, 50, 100, 7912, 160, 160), (50, 10, 20, 30, 6, 4)):
        assert dprnn.num_chunks(L, K, P) == S, (L, P, K)
        assert int(dprnn.chunk_counts(torch.tensor(n), K, P)) == S_b, (n, P, K)
    assert dprnn.chunk_counts([20, 14, 9], 6, 3).tolist() == [8, 6, 4]


def test_auto_window():
    from padertorch_amd.modules import DPRNN
    net = DPRNN(8, 8, 'auto', 'auto', 1)
    assert net.calculate_window_and_hop_size(torch.zeros(1, 18, 8)) == (6, 3)
    assert net.calculate_window_and_hop_size(torch.zeros(1, 18, 8), torch.tensor([18])) == (6, 3)
    with pytest.raises(AssertionError, match='not supported'):
        net.calculate_window_and_hop_size(torch.zeros(2, 18, 8), torch.tensor([18, 9]))
    with pytest.raises(AssertionError, match='Set both'):
        DPRNN(8, 8, 'auto', 3, 1).calculate_window_and_hop_size(torch.zeros(1, 18, 8))
    assert DPRNN(8, 8, 6, 3, 1).calculate_window_and_hop_size(torch.zeros(1, 18, 8)) == (6, 3)


def test_refusals():
    from padertorch_amd.modules import DPRNN, overlap_add, segment
    from padertorch_amd.ops import dprnn
    for kind in ('gru', 'bgru', 'cnn'):
        with pytest.raises(NotImplementedError, match='no HIP kernel'):
            DPRNN(8, 8, 6, 3, 1, inter_chunk_type=kind)
        with pytest.raises(NotImplementedError, match='no HIP kernel'):
            DPRNN(8, 8, 6, 3, 1, intra_chunk_type=kind)
    with pytest.raises(ValueError, match='Unknown rnn_type'):
        DPRNN(8, 8, 6, 3, 1, intra_chunk_type='rnn')
    DPRNN(8, 129, 6, 3, 1)                  # above 128 units W_hh is streamed, not refused
    with pytest.raises(NotImplementedError, match='at most 1536'):
        DPRNN(8, 1537, 6, 3, 1)
    net = DPRNN(8, 8, 6, 3, 1)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        net(torch.zeros(2, 20, 8), [20, 9])
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        segment(torch.zeros(1, 20, 8), 3, 6)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        overlap_add(torch.zeros(1, 8, 6, 4), 3)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        dprnn.chunk_lstm(torch.zeros(4, 8), torch.zeros(1, 3, dtype=torch.int32), 4, net.dprnn_blocks[0].intra_chunk_rnn.rnn)
    with pytest.raises(NotImplementedError, match='float32 only'):
        dprnn.segment_rows(torch.zeros(1, 20, 8, dtype=torch.float64), 6, 3)
    with pytest.raises(ValueError, match='sequence'):
        net(torch.zeros(2, 20, 7))


def test_ops_have_a_cuda_kernel_only():
    import padertorch_amd  # noqa: F401
    for n in OPS:
        assert getattr(torch.ops.ptmi, n).default._schema.name == f'ptmi::{n}'
        assert torch._C._dispatch_has_kernel_for_dispatch_key(f'ptmi::{n}', 'CUDA')
        assert not torch._C._dispatch_has_kernel_for_dispatch_key(f'ptmi::{n}', 'CPU')


def test_header_library_and_signatures_agree():
    import ctypes
    from padertorch_amd import _lib
    from padertorch_amd.build import build
    text = re.sub(r'/\*.*?\*/', '', (REPO / 'include' / 'ptmi.h').read_text(), flags=re.S)
    names = set(re.findall(r'\b(ptmi_(?:dprnn|chunk_lstm)_[a-z0-9_]+)\s*\(', text))
    assert len(names) == 13 and names == {n for n in _lib.SIGNATURES if n.startswith(('ptmi_dprnn_', 'ptmi_chunk_lstm_'))}
    build()
    lib = ctypes.CDLL(str(_lib.LIB_PATH))
    for n in names:
        assert hasattr(lib, n), n
    lib = _lib.load()
    assert lib.ptmi_chunk_lstm_max_hidden() == 1536 and lib.ptmi_chunk_lstm_max_resident_hidden() == 128 and lib.ptmi_chunk_lstm_tile() == 4
    from padertorch_amd.ops import dprnn
    assert dprnn.MAX_HIDDEN == lib.ptmi_chunk_lstm_max_hidden()
    for L, K, P in ((5, 4, 2), (5, 4, 3), (5, 4, 1), (7912, 100, 50), (3, 8, 4), (1, 1, 1)):
        assert lib.ptmi_dprnn_num_chunks(L, K, P) == dprnn.num_chunks(L, K, P)
