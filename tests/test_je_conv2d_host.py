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


# ------------------------------------------------------------------------------------ the planner paths of test_gpu_je_conv2d_paths.py
def c2_plan(Cs, NS, Co, NQ, K, stride, dilation):
    """``c2_plan`` of ``csrc/je_conv2d.hip`` restated: the derived values of a launch with ``NS`` sources of ``Cs`` channels and ``NQ``
    outputs of ``Co`` channels whose windows move by ``stride`` (8 x 16 output pixels a workgroup, 64 KB of LDS); None: refused."""
    Cp = -(-Cs // 8) * 8
    HF, HT = (7 * stride[0] + (K[0] - 1) * dilation[0] + 1, 15 * stride[1] + (K[1] - 1) * dilation[1] + 1)
    if HF * HT > 8192:
        return None
    cv = NS * Cp
    CC = 32 if cv >= 32 else (16 if cv >= 16 else 8)
    while CC > 8 and HF * HT * (4 * CC + 16) > 64 * 1024:
        CC //= 2
    if HF * HT * (4 * CC + 16) > 64 * 1024:
        return None
    return dict(Cp=Cp, HF=HF, HT=HT, CC=CC, NCH=-(-cv // CC), KS=(K[0] * K[1] * (CC // 8) + 3) // 4, tiles_n=-(-Co // (64 // NQ)),
                lds=HF * HT * (4 * CC + 16))


def launches(c_in, c_out, kernel, kwargs, plane, B=2):
    """``{'fwd' / 'dx': (the 21 geometry values as ops.je_conv2d._Block2dFn and ops.library build them, the restated plan)}`` and the 17
    of the weight gradient for a ``Conv2d`` on ``plane``."""
    from padertorch_amd.contrib.je.modules import Conv2d, compute_pad_size
    kwargs = {k: v for k, v in kwargs.items() if k != 'residual'}
    net = Conv2d(c_in, c_out, kernel, **kwargs)
    F_out, T_out = (int(n) for n in net.get_output_shape((B, c_in, *plane))[2:])
    K, s, d = net.kernel_size, net.stride, net.dilation
    front = [compute_pad_size(k, dd, ss, p)[0] for k, dd, ss, p in zip(K, d, s, net.pad_type)]
    G = 2 if net.gated else 1
    back = [(k - 1) * dd - f for k, dd, f in zip(K, d, front)]
    return {'fwd': ([B, *plane, c_in, 1, 1, 1, F_out, T_out, c_out, G, *K, *s, *d, *front, c_in, c_out], c2_plan(c_in, 1, c_out, G, K, s, d)),
            'dx': ([B, F_out, T_out, c_out, G, *s, *plane, c_in, 1, *K, 1, 1, *d, *back, c_out, c_in], c2_plan(c_out, G, c_in, 1, K, (1, 1), d)),
            }, [B, *plane, c_in, F_out, T_out, c_out, G, *K, *s, *d, *front, c_in]


def pack_elems(geom):
    from padertorch_amd import _lib
    return _lib.load().ptmi_je_conv2d_pack_elems(_lib.int64s(*geom))


def wgrad_lds(geom):
    from padertorch_amd import _lib
    return _lib.load().ptmi_je_conv2d_wgrad_lds(_lib.int64s(*geom))


def test_planner_restatement_on_known_plans():
    """The restatement against plans worked out by hand from the kernel's comment (halo x pitch within 64 KB)."""
    assert c2_plan(8, 1, 16, 1, (3, 3), (1, 1), (1, 1)) == dict(Cp=8, HF=10, HT=18, CC=8, NCH=1, KS=3, tiles_n=1, lds=180 * 48)
    assert c2_plan(32, 1, 16, 1, (3, 3), (2, 2), (1, 1)) == dict(Cp=32, HF=17, HT=33, CC=16, NCH=2, KS=5, tiles_n=1, lds=561 * 80)
    assert c2_plan(16, 2, 8, 1, (3, 3), (1, 1), (1, 1)) == dict(Cp=16, HF=10, HT=18, CC=32, NCH=1, KS=9, tiles_n=1, lds=180 * 144)
    assert c2_plan(8, 1, 16, 1, (7, 7), (3, 3), (1, 1)) is None and 28 * 52 * 48 > 64 * 1024


def test_every_path_case_reaches_the_path_it_names():
    """For every case of the GPU table, forward and ``dx`` launch: the library plans what the restatement plans (the size of the packed
    weight planes says so), the plan is the one the case is named for, and the weight gradient takes the layer."""
    from test_gpu_je_conv2d_paths import BASE, EDGE_BLOCKS, EDGES, PATHS
    cases = {name: case for name, case in PATHS.items()}
    cases.update({f'plane {plane}': (*BASE, plane, {}) for plane in EDGES})
    cases.update({f'plane (9, 17), {name}': (8, 16, 3, kwargs, (9, 17), {}) for name, kwargs in EDGE_BLOCKS.items()})
    named = 0
    for name, (c_in, c_out, kernel, kwargs, plane, claims) in cases.items():
        planned, wgeom = launches(c_in, c_out, kernel, kwargs, plane)
        assert set(claims) <= set(planned), name
        for launch, (geom, plan) in planned.items():
            assert plan is not None, (name, launch)
            assert pack_elems(geom) == plan['tiles_n'] * plan['NCH'] * plan['KS'] * 8 * 64 * 8, (name, launch, plan)
            for key, value in claims.get(launch, {}).items():
                assert plan[key] == value, (name, launch, key, plan[key], value)
                named += 1
        assert 0 < wgrad_lds(wgeom) <= 96 * 1024, name
    assert named >= 40


def test_refused_geometries():
    """The forward planner's refusal (0 elements) and the weight gradient's own (0 bytes) - and its widest supported neighbour."""
    from test_gpu_je_conv2d_paths import PLANE, REFUSED_FORWARD, REFUSED_WGRAD, WIDEST_WGRAD
    planned, _ = launches(*REFUSED_FORWARD, PLANE)
    assert planned['fwd'][1] is None and pack_elems(planned['fwd'][0]) == 0
    planned, wgeom = launches(*REFUSED_WGRAD, PLANE)
    assert all(plan is not None and pack_elems(geom) > 0 for geom, plan in planned.values())          # forward and dx plan fine
    assert wgrad_lds(wgeom) == 0 and 2 * 64 * 136 * 2 + 2 * 64 * 15 * 31 * 2 == 153856 > 96 * 1024
    planned, wgeom = launches(*WIDEST_WGRAD, PLANE)
    assert all(plan is not None and pack_elems(geom) > 0 for geom, plan in planned.values()) and wgrad_lds(wgeom) == 94336
    from padertorch_amd import _lib
    assert _lib.load().ptmi_je_conv2d_wgrad_lds(None) == 0 and wgrad_lds([0] * 17) == 0


def test_max_pool_oracle_is_torchs_on_a_tie_free_input():
    """``max_pool64`` (the GPU tests' oracle where values tie) against ``F.max_pool2d`` on the padded and trimmed plane, where nothing
    ties: values, indices and the gradient."""
    import torch.nn.functional as F
    from padertorch_amd.contrib.je.modules import to_pair
    from test_gpu_je_conv2d import POOLS
    from test_gpu_je_conv2d_paths import max_pool64, max_pool64_backward, pool_geometry
    x0 = np.random.RandomState(8).randn(2, 5, 12, 21).astype(np.float32)
    for size, stride, pad in sorted({p[:3] for p in POOLS}, key=str) + [((2, 2), (3, 3), 'both'), ((3, 3), (1, 1), 'both')]:
        eff = to_pair(size if stride is None else stride)
        front, end, out = pool_geometry(x0.shape[2:], size, eff, pad)
        y, index = max_pool64(x0, size, eff, front, end)
        assert y.shape[2:] == out
        xc = torch.from_numpy(x0).double().requires_grad_()
        xp = F.pad(xc, (front[1], end[1], front[0], end[0]))
        xp = xp[:, :, :(out[0] - 1) * eff[0] + size[0], :(out[1] - 1) * eff[1] + size[1]]
        yc, ic = F.max_pool2d(xp, size, eff, return_indices=True)
        assert np.array_equal(y, yc.detach().numpy()) and np.array_equal(index, ic.numpy()), (size, stride, pad)
        r = np.random.RandomState(9).randn(*y.shape).astype(np.float32)
        want = torch.autograd.grad((yc * torch.from_numpy(r).double()).sum(), xc)[0].numpy()
        assert np.array_equal(max_pool64_backward(r, index, x0.shape[2:], size, eff, front), want), (size, stride, pad)
