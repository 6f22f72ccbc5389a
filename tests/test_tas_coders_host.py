"""TasEncoder / TasDecoder without a GPU: interface parity with the reference (constructor, attributes, state_dict, length
arithmetic: tests/golden/g13_tas_coders.npz), the refusals, and the registration of the kernels."""
import json
import re
from pathlib import Path

import numpy as np
import pytest
import torch

REPO = Path(__file__).resolve().parent.parent


@pytest.fixture(scope='module')
def g13():
    d = dict(np.load(REPO / 'tests' / 'golden' / 'g13_tas_coders.npz', allow_pickle=False))
    d['cases'] = json.loads(str(d['cases']))
    return d


def _coders(case):
    from padertorch_amd.contrib.examples.source_separation.tasnet import TasDecoder, TasEncoder
    L, N, stride, bias, _ = case
    kw = dict(window_length=L, feature_size=N, stride=stride, bias=bias)
    return TasEncoder(**kw), TasDecoder(**kw)


def test_classes_are_exported_with_the_reference_defaults():
    from padertorch_amd.contrib.examples.source_separation.tasnet import TasDecoder, TasEncoder
    from padertorch_amd.contrib.examples.source_separation.tasnet import tas_coders
    assert tas_coders.TasEncoder is TasEncoder and tas_coders.TasDecoder is TasDecoder
    for coder, name, shape in ((TasEncoder(), 'encoder_1d', (256, 1, 20)), (TasDecoder(), 'decoder_1d', (256, 1, 20))):
        assert (coder.window_length, coder.feature_size, coder.stride) == (20, 256, 10)
        assert {k: tuple(v.shape) for k, v in coder.state_dict().items()} == {f'{name}.weight': shape}
    assert isinstance(TasEncoder().encoder_1d, torch.nn.Conv1d) and isinstance(TasDecoder().decoder_1d, torch.nn.ConvTranspose1d)
    assert TasEncoder(16, 8, stride=4).stride == 4 and TasDecoder(16, 8, stride=4).decoder_1d.stride == (4,)


def test_state_dict_matches_the_reference_and_loads(g13):
    for i, case in enumerate(g13['cases']):
        enc, dec = _coders(case)
        for coder, prefix, short in ((enc, 'encoder_1d.', 'enc_'), (dec, 'decoder_1d.', 'dec_')):
            ref = {prefix + k[len(f'c{i}_' + short):]: torch.from_numpy(v) for k, v in g13.items() if k.startswith(f'c{i}_' + short)}
            assert ref and {k: v.shape for k, v in coder.state_dict().items()} == {k: v.shape for k, v in ref.items()}, (case, ref.keys())
            coder.load_state_dict(ref)          # strict
            for k, v in coder.state_dict().items():
                assert torch.equal(v, ref[k])
        assert (enc.encoder_1d.bias is not None) == case[3] == (dec.decoder_1d.bias is not None)
        assert dec.decoder_1d.bias is None or dec.decoder_1d.bias.shape == (1,)


def test_encoded_lengths_and_frames_match_the_reference(g13):
    from padertorch_amd.ops import tas
    for i, case in enumerate(g13['cases']):
        enc, _ = _coders(case)
        L, N, stride, _, T = case
        got = enc.encoded_lengths(torch.from_numpy(g13[f'c{i}_lengths_in']), T)
        assert got.tolist() == g13[f'c{i}_lengths_out'].tolist(), case
        assert enc.encoded_lengths(None, T) is None
        B, n, frames = g13[f'c{i}_shapes'][0]
        assert (n, tas.tas_encoded_frames(T, L, enc.stride)) == (N, frames), case
        assert (frames - 1) * enc.stride + L == g13[f'c{i}_shapes'][1][1]
    # the issue's table at full length: L 16 at 32000 samples, and the stride-independent quirk
    assert tas.tas_encoded_frames(32000, 16, 8) == 3999
    assert tas.tas_encoded_lengths(torch.tensor([32000, 31900, 31850]), 32000, 16).tolist() == [3999, 3986, 3980]
    assert tas.tas_encoded_lengths(torch.tensor([1001, 901, 851]), 1001, 16).tolist() == [125, 112, 106]


def test_no_cpu_fallback_and_argument_checks():
    from padertorch_amd import ops
    from padertorch_amd.contrib.examples.source_separation.tasnet import TasDecoder, TasEncoder
    enc, dec = TasEncoder(4, 3), TasDecoder(4, 3)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        enc(torch.zeros(2, 100))
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        dec(torch.zeros(2, 3, 49))
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        dec.masked(torch.zeros(2, 2, 3, 49), torch.zeros(2, 3, 49))
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        ops.tas_encode(torch.zeros(2, 100), enc.encoder_1d.weight, None, 2, 4)
    with pytest.raises(AssertionError, match='1D and 2D input'):
        enc(torch.zeros(2, 3, 100))
    assert ops.tas_decode is ops.tas.tas_decode and ops.tas_masked_decode is ops.tas.tas_masked_decode


def test_every_tas_symbol_of_the_header_has_a_signature():
    from padertorch_amd import _lib
    text = re.sub(r'/\*.*?\*/', '', (REPO / 'include' / 'ptmi.h').read_text(), flags=re.S)
    names = set(re.findall(r'\b(ptmi_tas_[a-z0-9_]+)\s*\(', text))
    assert {'ptmi_tas_analysis', 'ptmi_tas_synthesis', 'ptmi_tas_wgrad', 'ptmi_tas_wgrad_workspace_elems',
            'ptmi_tas_masked_decode_backward'} <= names
    assert names == {n for n in _lib.SIGNATURES if n.startswith('ptmi_tas_')}


def test_tas_ops_have_a_cuda_kernel_only():
    import padertorch_amd  # noqa: F401
    for n in ('tas_analysis', 'tas_synthesis', 'tas_masked_decode_backward', 'tas_wgrad'):
        assert getattr(torch.ops.ptmi, n).default._schema.name == f'ptmi::{n}'
        assert torch._C._dispatch_has_kernel_for_dispatch_key(f'ptmi::{n}', 'CUDA')
        assert not torch._C._dispatch_has_kernel_for_dispatch_key(f'ptmi::{n}', 'CPU')
    with pytest.raises(NotImplementedError):
        torch.ops.ptmi.tas_analysis(torch.zeros(1, 8), torch.zeros(2, 4), None, 2, 3, True)
