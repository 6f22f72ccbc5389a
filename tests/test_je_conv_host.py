"""contrib/je's Conv1d / CNN1d / Pool1d without a GPU: the fp64 restatement tests/je_conv_ref.py against the reference's fp64 run
(tests/golden/g26_je_conv.npz), the shape and length functions against the recorded ones, strict state_dict loading, the freeze
bookkeeping and every NotImplementedError the modules promise."""
import importlib.util
import json
from pathlib import Path

import numpy as np
import pytest
import torch

import je_conv_ref as ref

GOLDEN = Path(__file__).resolve().parent / 'golden'
TIGHT = 1e-10          # fp64 against fp64: relative to max|want|


@pytest.fixture(scope='module')
def g26():
    d = dict(np.load(GOLDEN / 'g26_je_conv.npz', allow_pickle=False))
    spec = importlib.util.spec_from_file_location('make_golden_je_conv', GOLDEN / 'make_golden_je_conv.py')
    d['maker'] = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(d['maker'])             # for the seeded inputs and the constructors (the reference is not imported)
    return d


def build(g, case):
    from padertorch_amd.contrib.je import modules as je
    cls, args, kwargs = g['maker'].CASES[case]
    net = getattr(je, cls)(*args, **kwargs)
    keys = json.loads(str(g[case + '_keys']))
    net.load_state_dict({k: torch.from_numpy(g[f'{case}_p_{k}']) for k in keys}, strict=True)
    assert list(net.state_dict()) == keys
    return net


def near(name, got, want, tol=TIGHT, scale=None):
    got, want = torch.as_tensor(got).double(), torch.as_tensor(want).double()
    assert got.shape == want.shape, (name, got.shape, want.shape)
    scale = float(want.abs().max()) if scale is None else scale
    err = float((got - want).abs().max())
    assert err <= tol * scale, (name, err, scale)


def bias_scale(g, case, name):
    """The scale of a parameter gradient's gate: its own maximum, or - a convolution bias in front of a normalisation, zero in exact
    arithmetic - the maximum of its convolution's weight gradient (make_golden_je_conv.py)."""
    want = g[f'{case}_g64_{name}']
    scale = float(np.abs(want).max())
    if name.endswith('conv.bias'):
        wscale = float(np.abs(g[f'{case}_g64_{name[:-4]}weight']).max())
        if scale < g['maker'].ZERO_BIAS * wscale:
            return wscale
    return scale


@pytest.mark.parametrize('case', ['c0', 'c1', 'c2', 'c3', 'c4', 'n0', 'n1', 'n2'])
def test_restatement_equals_the_reference(g26, case):
    mk = g26['maker']
    net = build(g26, case).double()
    names = json.loads(str(g26[case + '_names']))
    assert names == [n for n, _ in net.named_parameters()]
    x = torch.from_numpy(mk.inputs(case)).double().requires_grad_()
    out = (ref.cnn1d if case.startswith('n') else ref.conv1d)(net, x, list(mk.LENGTHS))
    y = out[0]
    _, r0 = mk.inputs(case, tuple(y.shape))
    near(case + ' y', y.detach(), g26[case + '_y64'])
    assert np.array_equal(out[1], g26[case + '_len'])
    grads = torch.autograd.grad((y * torch.from_numpy(r0).double()).sum(), [x] + list(net.parameters()))
    near(case + ' dx', grads[0], g26[case + '_g64_x'], 1e-9)
    for n, got in zip(names, grads[1:]):
        near(f'{case} d {n}', got, g26[f'{case}_g64_{n}'], 1e-9, bias_scale(g26, case, n))
    if case == 'n0':
        assert np.array_equal(out[2][1].numpy(), g26['n0_idx1'])


def test_restatement_running_statistics_and_evaluation(g26):
    mk = g26['maker']
    net = build(g26, 'n0').double()
    x = torch.from_numpy(mk.inputs('n0')).double()
    for _ in range(2):
        ref.cnn1d(net, x, list(mk.LENGTHS), track=True)
    net.eval()
    with torch.no_grad():
        y = ref.cnn1d(net, x, list(mk.LENGTHS))[0]
    near('n0 evaluation', y, g26['n0e_y64'])
    state = net.state_dict()
    buffers = [k[len('n0e_b_'):] for k in g26 if k.startswith('n0e_b_')]
    assert buffers
    for k in buffers:
        near(k, state[k], g26['n0e_b_' + k])


@pytest.mark.parametrize('pad', ['both', 'front', 'end', None])
def test_restatement_pool(g26, pad):
    mk = g26['maker']
    x = torch.from_numpy(mk.pool_inputs(pad)).double().requires_grad_()
    y, idx = ref.pool(x, 3, 2, pad, True)
    near('y', y.detach(), g26[f'q_{pad}_y64'])
    assert np.array_equal(idx.numpy(), g26[f'q_{pad}_idx'])
    _, r0 = mk.pool_inputs(pad, tuple(y.shape))
    near('dx', torch.autograd.grad((y * torch.from_numpy(r0).double()).sum(), x)[0], g26[f'q_{pad}_g64_x'])
    assert np.array_equal(ref.out_lengths(mk.POOL_LENGTHS, 3, 1, 2, pad), g26[f'q_{pad}_len'])


@pytest.mark.parametrize('case', ['n0', 'n1', 'n2'])
def test_shapes_lengths_and_receptive_field(g26, case):
    mk = g26['maker']
    net = build(g26, case)
    shapes = net.get_shapes(input_shape=(mk.B, mk.C, mk.T))
    assert [[int(v) for v in s] for s in shapes] == json.loads(str(g26[case + '_shapes']))
    lens = net.get_sequence_lengths(input_sequence_lengths=np.asarray(mk.LENGTHS))
    assert [[int(v) for v in s] for s in lens] == json.loads(str(g26[case + '_seqlens']))
    assert np.array_equal(lens[-1], g26[case + '_len']) and lens[-1].dtype == np.int64
    assert np.array_equal(net.get_receptive_field(), g26[case + '_rf'])
    assert tuple(shapes[-1]) == g26[case + '_y64'].shape
    back = net.get_shapes(target_shape=shapes[-1])
    assert len(back) == len(shapes) and tuple(back[-1]) == tuple(shapes[-1])


def test_conv1d_shape_functions(g26):
    from padertorch_amd.contrib.je.modules import Conv1d, compute_pad_size
    mk = g26['maker']
    for case in ('c0', 'c1', 'c2', 'c3', 'c4'):
        net = build(g26, case)
        assert tuple(net.get_output_shape((mk.B, mk.C, mk.T))) == g26[case + '_y64'].shape
        assert np.array_equal(net.get_output_sequence_lengths(mk.LENGTHS), g26[case + '_len'])
    cnn = Conv1d(4, 20, 5, stride=2, pad_type=None)
    assert list(cnn.get_output_shape((5, 4, 103))) == [5, 20, 50]
    assert list(Conv1d(4, 20, 5, stride=2, pad_type='both').get_output_shape((5, 4, 103))) == [5, 20, 52]
    assert list(cnn.get_input_shape((5, 20, 50))) == [5, 4, 103]
    assert compute_pad_size(5, 2, 2, 'front') == (7, 1) and compute_pad_size(3, 1, 1, 'both') == (1, 1)
    assert compute_pad_size(4, 1, 1, 'both') == (1, 2) and compute_pad_size(3, 1, 3, 'end') == (0, 2)


def test_freeze_bookkeeping(g26):
    net = build(g26, 'n2')
    net.freeze(num_layers=1, freeze_norm_stats=False)
    assert not any(p.requires_grad for p in net.convs[0].parameters())
    assert all(p.requires_grad for p in net.convs[1].parameters())
    assert net.convs[0].norm.frozen_stats is False
    assert all(p.requires_grad for p in net.residual_skip_convs['0->2'].parameters())
    net.freeze(num_layers=2)
    assert not any(p.requires_grad for p in net.residual_skip_convs['0->2'].parameters())
    assert net.convs[1].norm.frozen_stats is True and net.convs[0].norm.frozen_stats is True
    assert all(p.requires_grad for p in net.convs[2].parameters())
    net.freeze()
    assert not any(p.requires_grad for p in net.parameters())
    other = build(g26, 'n0')
    other.freeze(0)
    assert all(p.requires_grad for p in other.parameters())


def test_what_is_not_built_raises():
    from padertorch_amd.contrib.je.modules import CNN1d, Conv1d, conv, conv_utils, map_activation_fn
    with pytest.raises(NotImplementedError, match='return_state'):
        Conv1d(4, 4, 3, return_state=True)
    with pytest.raises(NotImplementedError, match='return_state'):
        CNN1d(4, [4], 3, return_state=True)
    with pytest.raises(NotImplementedError, match='state'):
        Conv1d(4, 4, 3)(torch.zeros(1, 4, 8), state=torch.zeros(1, 4, 2))
    with pytest.raises(NotImplementedError, match='state'):
        CNN1d(4, [4], 3)(torch.zeros(1, 4, 8), state=[None])
    with pytest.raises(NotImplementedError, match='get_transpose_config'):
        CNN1d.get_transpose_config({'factory': CNN1d})
    for fn in ('softplus', 'gelu', torch.nn.Softplus(), torch.nn.functional.relu, torch.nn.PReLU(3)):
        with pytest.raises(NotImplementedError):
            map_activation_fn(fn)
        with pytest.raises(NotImplementedError):
            Conv1d(4, 4, 3, activation_fn=fn)
    with pytest.raises(NotImplementedError, match='shift'):
        Conv1d(4, 4, 3, norm='batch', norm_kwargs=dict(shift=False))
    for name in ('ConvTranspose1d', 'Conv2d', 'ConvTranspose2d', 'CNNTranspose1d', 'CNN2d', 'CNNTranspose2d', 'resnet50'):
        assert not hasattr(conv, name), name
    for name in ('Pool2d', 'Unpool1d', 'Unpool2d'):
        assert not hasattr(conv_utils, name), name
    with pytest.raises(RuntimeError, match='no CPU fallback'):          # and no fallback: a CPU tensor is refused, not computed
        Conv1d(4, 4, 3)(torch.zeros(1, 4, 8))
    assert type(map_activation_fn('linear')) is type(map_activation_fn(None)) is torch.nn.Identity
