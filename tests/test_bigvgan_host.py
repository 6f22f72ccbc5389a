"""The BigVGAN generator without a GPU: the fp64 restatement (tests/bigvgan_ref.py) against the reference's golden runs
(tests/golden/g23_bigvgan.npz), and the host side of the modules - parameter names, weight-norm folding on load, the vocoder's tag
arithmetic and its refusal to look anywhere but a local directory, the argument checks of the functional layer."""
import json
import socket

import pytest
import torch

import bigvgan_ref as ref


def bigvgan():
    from padertorch_amd.contrib.mk.synthesis.vocoder import nvidia_bigvgan
    return nvidia_bigvgan


def ops():
    from padertorch_amd.ops import bigvgan
    return bigvgan


@pytest.mark.parametrize('name', ref.case_names())
def test_restatement_reproduces_the_golden(name):
    """Every stored tensor of every case, to 1e-12 of its largest value: both sides are fp64, they differ in summation order only."""
    meta, x, want, _ = ref.case(name)
    got = ref.generator(ref.state(name), meta['h'], x)
    assert set(got) == set(want)
    assert list(got['y'].shape) == meta['out_shape']
    for q in meta['quantities']:
        assert got[q].dtype == torch.float64
        dev = ref.rel_dev(got[q], want[q])
        assert dev <= 1e-12, (name, q, dev)


def test_output_lengths_of_the_cases():
    g = ref.golden()['cases']
    assert g['amp1']['out_shape'] == [2, 1, 72] and g['one']['out_shape'] == [1, 1, 8] and g['odd']['out_shape'] == [1, 1, 36]
    assert g['pad_odd']['out_shape'] == [1, 1, 11]          # (5 - 1) 2 - 2 ((5 - 2) // 2) + 5: k - u odd, one sample more than 2 T


def test_fold_weight_norm_turns_the_normed_state_into_the_folded_one():
    """1e-6 relative: fp32 rounding of one normalisation (the reference folds with another order of the same three operations)."""
    pre, post = ref.state('k1', 'sd_wn'), ref.state('k1')
    folded = 0
    for key, w in post.items():
        if key + '_g' in pre:
            g, v = pre[key + '_g'], pre[key + '_v']
            assert not torch.equal(v, w)                     # g is not |v| in this case: the fold does something
            got = ops().fold_weight_norm(g, v)
            assert got.shape == w.shape and got.dtype == torch.float32
            assert ref.rel_dev(got, w) <= 1e-6, key
            assert ref.rel_dev(ref.fold_weight_norm(g.double(), v.double()), w) <= 1e-6, key
            folded += 1
        else:
            assert torch.equal(pre[key], w), key
    assert folded == 1 + 2 + 2 * 6 + 1                       # conv_pre, two up-samplers, two AMPBlock1 of six convolutions, conv_post
    with pytest.raises(ValueError):
        ops().fold_weight_norm(torch.ones(3), torch.ones(3, 2, 2))


@pytest.mark.parametrize('name', ['amp1', 'amp2', 'k1'])
def test_constructor_keys_are_the_references(name):
    meta = ref.golden()['cases'][name]
    m = bigvgan().BigVGAN(meta['h'])
    assert isinstance(m.resblocks[0], bigvgan().AMPBlock1 if meta['h']['resblock'] == '1' else bigvgan().AMPBlock2)
    state = ref.state(name)
    assert sorted(m.state_dict()) == sorted(state)
    assert {k: tuple(v.shape) for k, v in m.state_dict().items()} == {k: tuple(v.shape) for k, v in state.items()}
    assert all(not p.requires_grad for p in m.parameters())
    m.load_state_dict(state, strict=True)
    assert all(torch.equal(v, state[k]) for k, v in m.state_dict().items())
    m.remove_weight_norm()                                   # a no-op
    assert all(torch.equal(v, state[k]) for k, v in m.state_dict().items())
    assert m.use_tanh_at_final == meta['h']['use_tanh_at_final'] and (m.conv_post.bias is not None) == meta['h']['use_bias_at_final']


def test_weight_normed_state_dicts_load_folded():
    meta = ref.golden()['cases']['k1']
    pre, post = ref.state('k1', 'sd_wn'), ref.state('k1')
    renamed = {k.replace('weight_g', 'parametrizations.weight.original0').replace('weight_v', 'parametrizations.weight.original1'): v
               for k, v in pre.items()}
    assert any('parametrizations' in k for k in renamed)
    for spelling in (pre, renamed):
        m = bigvgan().BigVGAN(meta['h'])
        m.load_state_dict(spelling, strict=True)
        got = m.state_dict()
        assert sorted(got) == sorted(post)
        for k, v in post.items():
            assert ref.rel_dev(got[k], v) <= 1e-6, k
    m = bigvgan().BigVGAN(meta['h'])
    broken = dict(pre)
    del broken['conv_pre.weight_g']
    with pytest.raises(RuntimeError, match='conv_pre'):
        m.load_state_dict(broken, strict=True)


def test_defaults_and_unknown_settings():
    h = dict(ref.golden()['cases']['amp1']['h'])
    del h['use_tanh_at_final'], h['use_bias_at_final']
    m = bigvgan().BigVGAN(h, use_cuda_kernel=True)           # accepted, ignored
    assert m.use_tanh_at_final is True and m.use_bias_at_final is True and m.conv_post.bias is not None
    assert m.h.use_cuda_kernel is True and m.h['num_mels'] == 8
    assert not hasattr(m, 'push_to_hub') and not hasattr(m, 'save_pretrained')
    with pytest.raises(ValueError, match='resblock'):
        bigvgan().BigVGAN(dict(h, resblock='3'))
    with pytest.raises(NotImplementedError, match='activation'):
        bigvgan().BigVGAN(dict(h, activation='relu'))
    with pytest.raises(NotImplementedError, match='activation'):
        bigvgan().AMPBlock2(h, 4, activation=None)


def _no_network(monkeypatch):
    def refuse(*args, **kwargs):
        raise AssertionError('a network API was called')
    monkeypatch.setattr(socket, 'create_connection', refuse)
    monkeypatch.setattr(socket, 'getaddrinfo', refuse)
    monkeypatch.setattr(socket.socket, 'connect', refuse)


def test_vocoder_reads_a_local_directory_only(tmp_path, monkeypatch):
    from padertorch_amd.contrib.mk.synthesis.vocoder import Vocoder
    from padertorch_amd.contrib.mk.synthesis.vocoder.bigvgan import Vocoder as same
    assert Vocoder is same
    _no_network(monkeypatch)
    # the tag arithmetic of the reference, on its two documented examples
    with pytest.raises(FileNotFoundError) as e:
        Vocoder(base_dir=tmp_path)
    assert str(tmp_path / 'bigvgan_v2_44khz_128band_256x') in str(e.value)
    with pytest.raises(FileNotFoundError) as e:
        Vocoder(base_dir=tmp_path, sampling_rate=22000, mel_bands=80)
    assert str(tmp_path / 'bigvgan_v2_22khz_80band_256x') in str(e.value)
    with pytest.raises(FileNotFoundError) as e:
        Vocoder(base_dir=tmp_path, version=None, sampling_rate=24000, mel_bands=100, fmax=12000, upsampling_ratio=None)
    assert str(tmp_path / 'bigvgan_24khz_100band_12k') in str(e.value)
    with pytest.raises(FileNotFoundError) as e:
        Vocoder(base_dir=tmp_path, vocoder_tag='mine')
    assert str(tmp_path / 'mine') in str(e.value)
    (tmp_path / 'mine').mkdir()
    with pytest.raises(FileNotFoundError, match='config.json'):
        Vocoder(base_dir=tmp_path, vocoder_tag='mine')


def test_vocoder_loads_a_checkpoint_written_by_the_test(tmp_path, monkeypatch):
    from padertorch_amd.contrib.mk.synthesis.vocoder import Vocoder
    _no_network(monkeypatch)
    meta = ref.golden()['cases']['k1']
    d = tmp_path / 'bigvgan_v2_24khz_8band_8x'
    d.mkdir()
    (d / 'config.json').write_text(json.dumps(meta['h']))
    torch.save({'generator': ref.state('k1', 'sd_wn')}, d / 'bigvgan_generator.pt')
    v = Vocoder(base_dir=tmp_path, sampling_rate=24000, mel_bands=8, upsampling_ratio=8)
    assert v.sampling_rate == 24000 and v.vocoder_tag == 'bigvgan_v2_24khz_8band_8x' and not v.vocoder_model.training
    for k, w in ref.state('k1').items():
        assert ref.rel_dev(v.vocoder_model.state_dict()[k], w) <= 1e-6, k
    with pytest.raises(RuntimeError, match='no CPU fallback'):           # device='cpu' is the reference's default; the kernels need the GPU
        v(torch.zeros(8, 5))
    with pytest.raises(TypeError, match='2- or 3-dim'):
        v(torch.zeros(8))


def test_no_cpu_fallback():
    o = ops()
    x, w = torch.zeros(1, 4, 9), torch.zeros(6, 4, 3)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        o.conv1d(x, w)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        o.conv_transpose1d(x, torch.zeros(4, 2, 4), torch.zeros(2), 2)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        o.conv_post(x, torch.zeros(1, 4, 7))
    meta = ref.golden()['cases']['k1']
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        bigvgan().BigVGAN(meta['h'])(torch.zeros(1, 8, 4))
    import padertorch_amd  # noqa: F401
    for name in ('bigvgan_taps_', 'bigvgan_conv_direct_', 'bigvgan_ola', 'bigvgan_post'):
        assert torch._C._dispatch_has_kernel_for_dispatch_key(f'ptmi::{name}', 'CUDA')
        assert not torch._C._dispatch_has_kernel_for_dispatch_key(f'ptmi::{name}', 'CPU')


def test_inference_only():
    o = ops()
    x, w = torch.zeros(1, 4, 9), torch.zeros(6, 4, 3)
    with pytest.raises(RuntimeError, match='inference only'):
        o.conv1d(x.clone().requires_grad_(True), w)
    with pytest.raises(RuntimeError, match='inference only'):
        o.conv1d(x, w.clone().requires_grad_(True))
    with pytest.raises(RuntimeError, match='inference only'):
        o.conv_transpose1d(x.clone().requires_grad_(True), torch.zeros(4, 2, 4), torch.zeros(2), 2)
    with pytest.raises(RuntimeError, match='inference only'):
        o.conv_post(x.clone().requires_grad_(True), torch.zeros(1, 4, 7))
    with torch.no_grad(), pytest.raises(RuntimeError, match='no CPU fallback'):      # grad mode off: not this error
        o.conv1d(x.clone().requires_grad_(True), w)


def test_argument_checks():
    o = ops()
    x, w = torch.zeros(1, 4, 9), torch.zeros(6, 4, 3)
    with pytest.raises(TypeError, match='float32'):
        o.conv1d(x.double(), w.double())
    with pytest.raises(TypeError, match='float32'):
        o.conv_post(x.half(), torch.zeros(1, 4, 7).half())
    with pytest.raises(ValueError):
        o.conv1d(x[0], w)
    with pytest.raises(ValueError, match='input channels'):
        o.conv1d(x, torch.zeros(6, 5, 3))
    with pytest.raises(ValueError, match='even'):
        o.conv1d(x, torch.zeros(6, 4, 4))
    with pytest.raises(ValueError, match='bias'):
        o.conv1d(x, w, torch.zeros(5))
    with pytest.raises(ValueError, match='residual'):
        o.conv1d(x, w, residual=x)
    with pytest.raises(ValueError, match='accumulate'):
        o.conv1d(x, w, accumulate=True)
    with pytest.raises(ValueError, match='path'):
        o.conv1d(x, w, path='fast')
    wide = o.DIRECT_MAX_CHANNELS + 1
    with pytest.raises(ValueError, match='direct'):
        o.conv1d(torch.zeros(1, wide, 9), torch.zeros(2, wide, 3), path='direct')
    with pytest.raises(ValueError, match='direct'):
        o.conv1d(x, torch.zeros(6, 4, 13), path='direct')
    with pytest.raises(ValueError, match='stride'):
        o.conv_transpose1d(x, torch.zeros(4, 2, 16), None, 9)
    with pytest.raises(ValueError, match='shorter'):
        o.conv_transpose1d(x, torch.zeros(4, 2, 3), None, 4)
    with pytest.raises(ValueError):
        o.conv_post(x, torch.zeros(2, 4, 7))
    with pytest.raises(ValueError, match='kernel size'):
        o.conv_post(x, torch.zeros(1, 4, 6))
    assert o.choose_path(o.DIRECT_MAX_CHANNELS + 1, 3, 1) == 'gemm' and o.choose_path(8, 13, 1) == 'gemm'
    assert o.direct_ok(o.DIRECT_MAX_CHANNELS, 11, 5) and not o.direct_ok(8, 11, 13)


def test_the_kernels_refuse_unsupported_geometry_before_touching_the_device():
    """PTMI_E_INVALID (-1) from every entry point (a non-null pointer stands in for the device buffers: nothing is launched)."""
    from padertorch_amd import _lib
    from padertorch_amd.build import build
    build()
    lib = _lib.load()
    p = 256
    assert lib.ptmi_bigvgan_direct_max_channels() == ops().DIRECT_MAX_CHANNELS
    assert lib.ptmi_bigvgan_tile(0) == ops().TAPS_TILE and lib.ptmi_bigvgan_tile(1) == ops().DIRECT_TILE
    for c_in, k, d in ((1, 1, 1), (128, 11, 12), (129, 3, 1), (8, 13, 1), (8, 4, 1), (8, 11, 13), (8, 3, 64), (8, 3, 65)):
        assert bool(lib.ptmi_bigvgan_direct_ok(c_in, k, d)) == ops().direct_ok(c_in, k, d), (c_in, k, d)
    assert lib.ptmi_bigvgan_ola_out_len(5, 5, 2) == 11 and lib.ptmi_bigvgan_ola_out_len(9, 8, 4) == 36
    assert lib.ptmi_bigvgan_ola_out_len(5, 16, 9) == -1 and lib.ptmi_bigvgan_ola_out_len(5, 3, 4) == -1
    assert _lib.call('ptmi_bigvgan_taps', p, None, None, 1, 4, 8, 4, 1, 1.0, 0, p, None, accept=(-1,)) == -1           # even K
    assert _lib.call('ptmi_bigvgan_taps', None, None, None, 1, 4, 8, 3, 1, 1.0, 0, p, None, accept=(-1,)) == -1
    assert _lib.call('ptmi_bigvgan_conv_direct', p, p, None, None, 1, 4, 4, 8, 4, 1, 1.0, 0, p, None, accept=(-1,)) == -1    # even K
    assert _lib.call('ptmi_bigvgan_conv_direct', p, p, None, None, 1, 4, 4, 8, 13, 1, 1.0, 0, p, None, accept=(-1,)) == -1   # K > 11
    assert _lib.call('ptmi_bigvgan_conv_direct', p, p, None, None, 1, 129, 4, 8, 3, 1, 1.0, 0, p, None, accept=(-1,)) == -1  # too wide
    assert _lib.call('ptmi_bigvgan_conv_direct', p, p, None, None, 1, 4, 4, 8, 11, 13, 1.0, 0, p, None, accept=(-1,)) == -1  # halo 65
    assert _lib.call('ptmi_bigvgan_ola', p, None, 1, 4, 8, 18, 9, p, None, accept=(-1,)) == -1                        # u > 8
    assert _lib.call('ptmi_bigvgan_ola', p, None, 1, 4, 8, 3, 4, p, None, accept=(-1,)) == -1                         # k < u
    assert _lib.call('ptmi_bigvgan_post', p, p, None, 1, 4, 8, 6, 1, p, None, accept=(-1,)) == -1                     # even K
    assert _lib.call('ptmi_bigvgan_post', p, p, None, 1, 4, 8, 13, 1, p, None, accept=(-1,)) == -1                    # K > 11
