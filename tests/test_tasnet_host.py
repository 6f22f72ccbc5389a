"""TasNet without a GPU: construction and state_dict parity with the reference (tests/golden/g15_tasnet.npz), the refusals, the length
arithmetic, the surface the reference Trainer touches, and the review helpers ``summary.audio`` / ``summary.review_dict`` against what
the reference's return."""
import json
import re
from pathlib import Path

import numpy as np
import pytest
import torch

REPO = Path(__file__).resolve().parent.parent


@pytest.fixture(scope='module')
def g15():
    d = dict(np.load(REPO / 'tests' / 'golden' / 'g15_tasnet.npz', allow_pickle=False))
    d['cases'] = json.loads(str(d['cases']))
    return d


def _net(c, **kw):
    from padertorch_amd.contrib.examples.source_separation.tasnet import TasDecoder, TasEncoder, TasNet
    from padertorch_amd.modules import ConvNet
    args = dict(mask=c['mask'], output_nonlinearity=c['nonlinearity'], num_speakers=c['K'], additional_out_size=c['A'])
    args.update(kw)
    return TasNet(TasEncoder(c['L'], c['n_enc'], c['stride']),
                  ConvNet(input_size=c['sep_in'], num_blocks=c['blocks'], num_repeats=c['repeats'], hidden_channels=c['hidden'],
                          kernel_size=3, norm=c['norm']),
                  TasDecoder(c['L'], c['n_dec'], c['stride']), **args)


def test_constructor_is_the_references(g15):
    import padertorch_amd as pta
    from padertorch_amd.contrib.examples.source_separation.tasnet import TasDecoder, TasEncoder, TasNet
    from padertorch_amd.modules import ConvNet
    net = TasNet(TasEncoder(16, 256), ConvNet(256), TasDecoder(16, 256))
    assert isinstance(net, pta.Model) and net.mask is True and net.num_speakers == 2 and net.additional_out_size == 0
    assert net.sample_rate == 8000 and isinstance(net.output_nonlinearity, torch.nn.Sigmoid) and net.return_encoded_out is False
    assert isinstance(net.encoded_input_norm, torch.nn.LayerNorm) and tuple(net.encoded_input_norm.weight.shape) == (256,)
    assert tuple(net.input_proj.weight.shape) == (256, 256, 1) and tuple(net.output_proj.weight.shape) == (512, 256, 1)
    assert isinstance(net.output_prelu, torch.nn.PReLU) and net.output_prelu.weight.numel() == 1
    with pytest.raises(AssertionError, match='features sizes must match'):
        TasNet(TasEncoder(16, 10), ConvNet(8, 1, 1, 16), TasDecoder(16, 6))
    TasNet(TasEncoder(16, 10), ConvNet(8, 1, 1, 16), TasDecoder(16, 6), mask=False)          # allowed without masking
    prelu = _net(g15['cases'][0], output_nonlinearity='prelu')
    assert 'output_nonlinearity.weight' in prelu.state_dict()
    net.flatten_parameters()                                                               # ConvNet has none: a no-op


def test_state_dict_matches_the_reference_and_loads_strictly(g15):
    for i, c in enumerate(g15['cases']):
        net = _net(c)
        keys = json.loads(str(g15[f'c{i}_keys']))
        ref = {k: torch.from_numpy(g15[f'c{i}_p_{k}']) for k in keys}
        own = net.state_dict()
        assert list(own) == keys, i
        assert {k: tuple(v.shape) for k, v in own.items()} == {k: tuple(v.shape) for k, v in ref.items()}, i
        net.load_state_dict(ref, strict=True)
        assert [n for n, _ in net.named_parameters()] == json.loads(str(g15[f'c{i}_names']))
        assert float(g15[f'c{i}_margin']) >= 1e-5


def test_softmax_and_callables_are_refused(g15):
    with pytest.raises(NotImplementedError, match='legacy'):
        _net(g15['cases'][0], output_nonlinearity='softmax')
    with pytest.raises(NotImplementedError, match='callables'):
        _net(g15['cases'][0], output_nonlinearity=torch.nn.Sigmoid)


def test_no_cpu_fallback_and_dtypes(g15):
    from padertorch_amd.ops import tasnet as glue
    c = g15['cases'][0]
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        _net(c)(dict(y=torch.zeros(c['B'], c['T']), num_samples=c['num_samples']))
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        glue.entry_norm(torch.zeros(1, 4, 8), torch.ones(4), torch.zeros(4))
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        glue.prelu_rows(torch.zeros(3, 4), torch.ones(1))
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        glue.mask_head(torch.zeros(1, 4, 8), 2, 4)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        glue.center(torch.zeros(2, 1, 8), 8)
    with pytest.raises(ValueError, match='activation'):
        glue.mask_head(torch.zeros(1, 4, 8), 2, 4, activation='softmax')
    for name in ('tasnet_entry_norm_forward', 'tasnet_entry_norm_backward', 'tasnet_prelu_forward', 'tasnet_prelu_backward',
                 'tasnet_mask_head_forward', 'tasnet_mask_head_backward', 'tasnet_center'):
        assert torch._C._dispatch_has_kernel_for_dispatch_key(f'ptmi::{name}', 'CUDA')
        assert not torch._C._dispatch_has_kernel_for_dispatch_key(f'ptmi::{name}', 'CPU')
    with pytest.raises(NotImplementedError):
        torch.ops.ptmi.tasnet_prelu_forward(torch.zeros(4), torch.ones(1))


def test_fp64_is_refused():
    from padertorch_amd.ops import tasnet as glue
    with pytest.raises(NotImplementedError, match='float32 only'):
        glue.entry_norm(torch.zeros(1, 4, 8, dtype=torch.float64), torch.ones(4, dtype=torch.float64), torch.zeros(4, dtype=torch.float64))
    with pytest.raises(NotImplementedError, match='float32 only'):
        glue.prelu_rows(torch.zeros(3, 4, dtype=torch.float64), torch.ones(1))
    with pytest.raises(NotImplementedError, match='float32 only'):
        glue.mask_head(torch.zeros(1, 4, 8, dtype=torch.float64), 2, 4)
    with pytest.raises(NotImplementedError, match='float32 only'):
        glue.center(torch.zeros(2, 1, 8, dtype=torch.float16), 8)


def test_every_tasnet_symbol_of_the_header_has_a_signature():
    from padertorch_amd import _lib
    text = re.sub(r'/\*.*?\*/', '', (REPO / 'include' / 'ptmi.h').read_text(), flags=re.S)
    names = set(re.findall(r'\b(ptmi_tasnet_[a-z0-9_]+)\s*\(', text))
    assert len(names) == 10 and names == {n for n in _lib.SIGNATURES if n.startswith('ptmi_tasnet_')}


def test_length_arithmetic(g15):
    from padertorch_amd.ops import tas
    for i, c in enumerate(g15['cases']):
        got = _net(c).encoder.encoded_lengths(torch.tensor(c['num_samples']), c['T'])
        assert got.tolist() == g15[f'c{i}_lengths'].tolist(), i
        stride = c['L'] // 2 if c['stride'] is None else c['stride']
        assert max(got.tolist()) <= tas.tas_encoded_frames(c['T'], c['L'], stride)


def test_model_surface_the_reference_trainer_touches(g15):
    m = _net(g15['cases'][0])
    assert isinstance(m, torch.nn.Module)
    for name in ('example_to_device', 'review', 'modify_summary', 'forward', 'loss', 'flatten_parameters'):
        assert callable(getattr(m, name)), name
    assert m.create_snapshot is False
    m.create_snapshot = True
    assert m.create_snapshot is True
    ex = dict(a=np.arange(3, dtype=np.float32), b=[np.ones(2, dtype=np.float32)], c='text')
    moved = m.example_to_device(ex, 'cpu')
    assert torch.is_tensor(moved['a']) and torch.is_tensor(moved['b'][0]) and moved['c'] == 'text'
    summary = dict(scalars=dict(loss=[1., 3.]), histograms={}, images={})
    assert m.modify_summary(summary)['scalars']['loss'] == 2.


def test_summary_helpers_against_the_reference(g15):
    from padertorch_amd import summary
    sig = g15['audio_in']
    a, rate = summary.audio(signal=torch.from_numpy(sig[0]), sampling_rate=8000)
    assert rate == int(g15['audio_rate']) == 8000 and a.dtype == g15['audio_out'].dtype
    np.testing.assert_array_equal(a, g15['audio_out'])
    assert abs(float(np.abs(a).max()) - 0.95) < 1e-6
    a, rate = summary.audio(signal=sig, batch_first=True, normalize=False)
    assert rate == int(g15['audio_rate_default']) == 16000
    np.testing.assert_array_equal(a, g15['audio_out_batch_first'])
    np.testing.assert_array_equal(summary.audio(signal=sig.T)[0], g15['audio_out_batch_second'])
    np.testing.assert_array_equal(summary.audio(signal=np.zeros(4, np.float32))[0], g15['audio_out_zeros'])
    with pytest.raises(ValueError, match='Complex'):
        summary.audio(np.zeros(4, np.complex64))
    review = summary.review_dict(losses={'a': torch.tensor(1.)}, audios={'b': (sig[0], 8000)})
    assert list(review) == json.loads(str(g15['review_keys']))
    with pytest.raises(AssertionError):
        summary.review_dict(loss=torch.tensor(1.), losses={'a': torch.tensor(1.)})
    with pytest.raises(AssertionError):
        summary.review_dict(audios={})
