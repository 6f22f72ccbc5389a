"""BigVGAN's anti-aliased activation, everything that needs no GPU: the filter design, the length arithmetic, the modules' names, the
restatement (tests/anti_alias_ref.py) against the reference's fp64 golden runs (tests/golden/g21_anti_alias.npz), the argument checks and
the C ABI."""
import math
import re
from pathlib import Path

import numpy as np
import pytest
import torch

import anti_alias_ref as ref

REPO = Path(__file__).resolve().parent.parent


def bigvgan():
    from padertorch_amd.contrib.mk.synthesis.vocoder import nvidia_bigvgan
    return nvidia_bigvgan


def test_filters_match_the_reference():
    """Ours are rounded once from fp64, the reference's are built in fp32: one fp32 ulp of the largest tap (< 0.5: 2^-24 .. 2^-23 -> 2e-7)."""
    from padertorch_amd.ops.anti_alias import kaiser_sinc_filter1d
    g = ref.golden()
    for i, (cutoff, half_width, k) in enumerate(g['filter_args']):
        f = kaiser_sinc_filter1d(float(cutoff), float(half_width), int(k))
        assert f.dtype == torch.float32 and tuple(f.shape) == (1, 1, int(k))
        dev = float(np.abs(f.numpy().astype(np.float64) - g[f'filters_{i}'].astype(np.float64)).max())
        print(f'filter {i} ({cutoff:.4g}, {half_width:.4g}, {int(k)}): max deviation {dev:.3g}')
        assert dev <= 2e-7
        assert abs(float(f.double().sum()) - 1) < 1e-6


def test_cutoff_zero_gives_zeros():
    from padertorch_amd.ops.anti_alias import kaiser_sinc_filter1d
    for k in (7, 12):
        f = kaiser_sinc_filter1d(0, 0.3, k)
        assert tuple(f.shape) == (1, 1, k) and not f.any()


@pytest.mark.parametrize('r,k,d,dk', [(2, 12, 2, 12), (3, 18, 3, 18), (2, 7, 2, 9), (4, 8, 2, 12), (1, 12, 1, 12), (3, 18, 2, 5)])
def test_length_arithmetic(r, k, d, dk):
    """``r T`` behind the up-sampler, ``ceil(U / d)`` behind the padded low-pass - in the C ABI and in the restatement."""
    from padertorch_amd import _lib
    lib = _lib.load()
    for T in (1, 2, 5, 37, 1025):
        U = r * T
        assert lib.ptmi_anti_alias_out_len(T, r, k, 1, 0, 1) == U
        assert lib.ptmi_anti_alias_out_len(T, r, k, d, dk, 1) == math.ceil(U / d)
        assert lib.ptmi_anti_alias_out_len(U, 1, 0, d, dk, 1) == math.ceil(U / d)
        if U >= dk:
            assert lib.ptmi_anti_alias_out_len(U, 1, 0, d, dk, 0) == (U - dk) // d + 1
        x = torch.zeros(1, 1, T, dtype=torch.float64)
        u = ref.upsample(x, torch.ones(k, dtype=torch.float64), r)
        assert u.shape[-1] == U and ref.lowpass(u, torch.ones(dk, dtype=torch.float64), d).shape[-1] == math.ceil(U / d)


def test_state_dict_names_and_strict_load():
    """The reference's buffer and parameter names; a state dict holding the golden (reference) filters loads strictly, and the loaded
    filters are the ones in the buffers the kernel reads."""
    bv = bigvgan()
    g = ref.golden()
    for cls, keys, case in ((bv.Snake, 'keys_snake', 'd37_snake'), (bv.SnakeBeta, 'keys_snakebeta', 'd37_beta')):
        m = bv.Activation1d(cls(4, alpha_logscale=True))
        assert list(m.state_dict()) == g[keys]
        _, t = ref.case_tensors(case)
        state = {'act.alpha': t['alpha'], 'upsample.filter': t['up_filter'], 'downsample.lowpass.filter': t['down_filter']}
        if 'beta' in t:
            state['act.beta'] = t['beta']
        m.load_state_dict(state, strict=True)
        assert torch.equal(m.upsample.filter, t['up_filter']) and torch.equal(m.downsample.lowpass.filter, t['down_filter'])
        assert m.upsample.filter.dtype == torch.float32 and tuple(m.upsample.filter.shape) == (1, 1, 12)
    frozen = bv.SnakeBeta(3, alpha_trainable=False)
    assert not frozen.alpha.requires_grad and not frozen.beta.requires_grad
    assert bv.Snake(2, alpha=3.0).alpha.tolist() == [3.0, 3.0] and bv.Snake(2, alpha=3.0, alpha_logscale=True).alpha.tolist() == [0.0, 0.0]
    up = bv.UpSample1d(3)
    assert (up.kernel_size, up.pad, up.pad_left, up.pad_right, up.stride) == (18, 5, 22, 23, 3)
    low = bv.DownSample1d(2).lowpass
    assert (low.kernel_size, low.pad_left, low.pad_right, low.stride, low.padding, low.even) == (12, 5, 6, 2, True, True)


@pytest.mark.parametrize('case', ref.activation_cases())
def test_restatement_reproduces_the_golden(case):
    meta, t = ref.case_tensors(case)
    got = ref.run(t['x'], t['alpha'], t.get('beta'), t['up_filter'], t['down_filter'], t['w'], meta['up_ratio'], meta['down_ratio'],
                  meta['logscale'])
    for q in ('y', 'dx', 'dalpha', 'dbeta'):
        if q in t:
            dev = ref.rel_dev(got[q], t[q])
            print(f'{case} {q}: {dev:.3g}')
            assert dev <= 1e-12, (case, q, dev)
    assert ('dbeta' in t) == (meta['cls'] == 'SnakeBeta')


def test_restatement_reproduces_the_stand_alone_goldens():
    for case, fn in (('up3', lambda x, f: ref.upsample(x, f, 3)), ('down2', lambda x, f: ref.lowpass(x, f, 2)),
                     ('down3', lambda x, f: ref.lowpass(x, f, 3)), ('lp7', lambda x, f: ref.lowpass(x, f, 1, padding=False))):
        _, t = ref.case_tensors(case)
        x = t['x'].double().requires_grad_(True)
        y = fn(x, t['filter'].double().reshape(-1))
        (y * t['w'].double()).sum().backward()
        assert ref.rel_dev(y, t['y']) <= 1e-12 and ref.rel_dev(x.grad, t['dx']) <= 1e-12, case


def test_argument_checks():
    bv = bigvgan()
    from padertorch_amd.ops import anti_alias as aa
    x = torch.zeros(1, 3, 8)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        bv.Activation1d(bv.SnakeBeta(3))(x)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        bv.Snake(3)(x)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        bv.UpSample1d(2)(x)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        bv.LowPassFilter1d(0.25, 0.3, stride=2)(x)
    with pytest.raises(ValueError, match='kernel size'):
        bv.UpSample1d(2, aa.MAX_TAPS + 2)
    with pytest.raises(ValueError, match='ratio'):
        bv.DownSample1d(aa.MAX_RATIO + 1, 12)
    with pytest.raises(ValueError, match='ratio'):
        bv.Activation1d(bv.Snake(3), up_ratio=aa.MAX_RATIO + 1, up_kernel_size=24)
    with pytest.raises(ValueError, match='kernel size'):
        aa.lowpass1d(x, torch.ones(1, 1, aa.MAX_TAPS + 1) / (aa.MAX_TAPS + 1), 2)
    with pytest.raises(ValueError, match='shorter than the ratio'):
        bv.UpSample1d(4, 2)
    bv.UpSample1d(aa.MAX_RATIO, aa.MAX_TAPS)                            # the bound itself is accepted
    with pytest.raises(NotImplementedError, match='replicat'):
        bv.LowPassFilter1d(0.25, 0.3, padding_mode='reflect')
    with pytest.raises(TypeError, match='float32'):
        bv.Activation1d(bv.SnakeBeta(3))(x.half())
    with pytest.raises(TypeError, match='float32'):
        aa.upsample1d(x.double(), aa.kaiser_sinc_filter1d(0.25, 0.3, 12))
    with pytest.raises(ValueError):
        bv.LowPassFilter1d(cutoff=0.6)


def test_c_abi_and_ops():
    from padertorch_amd import _lib
    from padertorch_amd.ops import anti_alias as aa
    text = re.sub(r'/\*.*?\*/', '', (REPO / 'include' / 'ptmi.h').read_text(), flags=re.S)
    lib = _lib.load()
    for name in ('ptmi_anti_alias_forward', 'ptmi_anti_alias_backward', 'ptmi_anti_alias_workspace_elems', 'ptmi_anti_alias_out_len',
                 'ptmi_anti_alias_tile'):
        assert re.search(rf'\b{name}\s*\(', text), name
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    assert lib.ptmi_anti_alias_tile(1) == aa.TILE and lib.ptmi_anti_alias_tile(0) == aa.TILE_GENERIC
    # two fp64 partials per workgroup; the backward tiles the INPUT
    assert lib.ptmi_anti_alias_workspace_elems(3, 5, 2 * aa.TILE + 3, 2, 12, 2, 12, 1) == 2 * 3 * 5 * 3
    assert lib.ptmi_anti_alias_workspace_elems(3, 5, aa.TILE_GENERIC + 1, 3, 18, 3, 18, 1) == 2 * 3 * 5 * 2
    assert lib.ptmi_anti_alias_out_len(10, 2, aa.MAX_TAPS + 1, 2, 12, 1) == -1 and lib.ptmi_anti_alias_out_len(10, 9, 54, 2, 12, 1) == -1
    for n in ('anti_alias_forward', 'anti_alias_backward'):
        assert getattr(torch.ops.ptmi, n).default._schema.name == f'ptmi::{n}'
        assert torch._C._dispatch_has_kernel_for_dispatch_key(f'ptmi::{n}', 'CUDA')
        assert not torch._C._dispatch_has_kernel_for_dispatch_key(f'ptmi::{n}', 'CPU')
    with pytest.raises(NotImplementedError):
        torch.ops.ptmi.anti_alias_forward(torch.zeros(1, 1, 4), None, None, None, None, 1, 1, True, False)
