"""``Conv2d`` / ``CNN2d`` / ``Pool2d`` / the hybrids: the bookkeeping that needs no GPU - shapes, lengths, receptive field and parameter
names against the values the reference stored in ``golden/g27``, the weight gradient's slab planner, and what is not built."""
import importlib.util
import json
from pathlib import Path

import numpy as np
import pytest
import torch


GOLDEN = Path(__file__).resolve().parent / 'golden'


@pytest.fixture(scope='module')
def g27():
    d = dict(np.load(GOLDEN / 'g27_je_conv2d.npz', allow_pickle=False))
    spec = importlib.util.spec_from_file_location('make_golden_je_conv2d', GOLDEN / 'make_golden_je_conv2d.py')
    d['maker'] = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(d['maker'])
    return d


@pytest.mark.parametrize('case', ['w0', 'w1', 'w2'])
def test_shapes_lengths_and_receptive_field(g27, case):
    """``get_shapes``, ``get_sequence_lengths``, ``get_receptive_field`` and the parameter names against what the reference stored."""
    from padertorch_amd.contrib.je.modules import CNN2d
    mk = g27['maker']
    _, args, kwargs = mk.CASES[case]
    net = CNN2d(*args, **kwargs)
    assert [[int(n) for n in s] for s in net.get_shapes(mk.SHAPE)] == json.loads(str(g27[case + '_shapes']))
    seqlens = json.loads(str(g27[case + '_seqlens']))
    assert [[int(n) for n in s] for s in net.get_sequence_lengths(mk.LENGTHS)] == seqlens
    assert np.array_equal(net.get_receptive_field(), g27[case + '_rf'])
    assert [n for n, _ in net.named_parameters()] == json.loads(str(g27[case + '_names']))
    assert list(net.state_dict()) == json.loads(str(g27[case + '_keys']))
    # the repeated vectors of one upload: B F entries at every stage, the last the output's
    rows = net._all_lengths(np.array(mk.LENGTHS), mk.SHAPE)
    assert len(rows[-1]) == 3 * g27[case + '_y64'].shape[2] and sorted(set(rows[-1].tolist())) == sorted(set(seqlens[-1]))


def test_pool2d_output_lengths_and_shapes(g27):
    from padertorch_amd.contrib.je.modules import Pool2d
    mk = g27['maker']
    for i, (kind, size, stride, pad) in enumerate(mk.POOLS):
        pool = Pool2d(kind, size, stride, pad)
        assert list(pool.geometry(mk.SHAPE[2:])[1]) == list(g27[f'p2_{i}_shape'][2:])
        assert np.array_equal(pool.output_lengths(mk.LENGTHS), g27[f'p2_{i}_len'])


def test_hybrid_configs_resolve_to_the_fixtures_constructors(g27):
    """``finalize_dogmatic_config`` from the partial configs: the channel counts between the stacks are the ones the fixture was built with."""
    from padertorch_amd.contrib.je.modules import CNN, CRNN
    mk = g27['maker']

    def partial(case, derived):
        kwargs = {k: (dict(v) if isinstance(v, dict) else v) for k, v in mk.CASES[case][1].items()}
        for part, key in derived:
            del kwargs[part][key]
        return kwargs
    cnn = CNN.from_config(partial('h0', [('cnn_1d', 'in_channels')]))
    crnn = CRNN.from_config(partial('h1', [('cnn_1d', 'in_channels'), ('rnn', 'input_size'), ('fcn', 'input_size')]))
    assert list(cnn.state_dict()) == json.loads(str(g27['h0_keys'])) and list(crnn.state_dict()) == json.loads(str(g27['h1_keys']))
    for k, v in list(cnn.state_dict().items()) + list(crnn.state_dict().items()):
        assert tuple(v.shape) == g27[('h0' if k.startswith('cnn_') else 'h1') + '_p_' + k].shape, k
    assert np.array_equal(cnn.get_seq_lens(mk.LENGTHS)[1][-1], g27['h0_len'])


def test_weight_gradient_slab_planner():
    from padertorch_amd.ops import je_conv2d as ops
    for args in ((2, 40, 150, 1, 16, 8, 9), (16, 128, 512, 1, 16, 16, 9), (16, 8, 512, 1, 256, 256, 9), (16, 1, 32, 1, 1024, 512, 9),
                 (1, 1, 1, 2, 5, 3, 1)):
        B, F_out, T_out, G, C_out, C_in, taps = args
        tiles = B * -(-F_out // 8) * -(-T_out // 16)
        slabs = ops.wgrad_slabs(*args)
        assert 1 <= slabs <= tiles and (slabs - 1) * -(-tiles // slabs) < tiles          # every range holds a tile
        assert slabs == 1 or slabs * 4 * G * C_out * C_in * taps <= ops.WGRAD_WORKSPACE_BYTES
    assert ops.wgrad_slabs(2, 40, 150, 1, 16, 8, 9) == 100 and ops.wgrad_slabs(16, 1, 32, 1, 1024, 512, 9) == 1


def test_what_is_not_built_raises():
    from padertorch_amd.contrib.je import modules as je
    with pytest.raises(NotImplementedError, match='return_state'):
        je.Conv2d(4, 4, 3, return_state=True)
    with pytest.raises(NotImplementedError, match='state'):
        je.Conv2d(4, 4, 3)(torch.zeros(1, 4, 8, 8), state=torch.zeros(1))
    with pytest.raises(NotImplementedError, match='state'):
        je.CNN2d(4, [4], 3)(torch.zeros(1, 4, 8, 8), state=[None])
    with pytest.raises(NotImplementedError, match='get_transpose_config'):
        je.CNN2d.get_transpose_config({})
    with pytest.raises(NotImplementedError):
        je.Conv2d(4, 4, 3, activation_fn='gelu')
    with pytest.raises(NotImplementedError, match='shift'):
        je.Conv2d(4, 4, 3, norm='batch', norm_kwargs=dict(shift=False))
    with pytest.raises(NotImplementedError, match='return_state'):
        je.CNN(je.CNN2d(1, [2], 3), je.CNN1d(2, [2], 3), return_state=True)
    with pytest.raises(NotImplementedError, match='get_transpose_config'):
        je.CNN.get_transpose_config({})
    with pytest.raises(NotImplementedError):
        je.CRNN(None, None, torch.nn.RNN(4, 4), None)
    for name in ('ConvTranspose2d', 'CNNTranspose2d', 'Unpool2d', 'resnet50', 'CNNTranspose'):
        assert not hasattr(je, name) and not hasattr(je.conv2d, name) and not hasattr(je.hybrid, name), name
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        je.Conv2d(4, 4, 3)(torch.zeros(1, 4, 8, 8))
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        je.Pool2d('max', 2)(torch.zeros(1, 4, 8, 8))
