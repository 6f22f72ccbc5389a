"""Host logic of OneAndRestPIT (no GPU): constructor checks, finalize_dogmatic_config, the reference's quirks as documented in the
model's docstring, the state_dict keys of tests/golden/g16_orpit.npz and the golden recipe's case table."""
import importlib.util
import json
from pathlib import Path

import numpy as np
import pytest
import torch

GOLDEN = Path(__file__).resolve().parent / 'golden'


@pytest.fixture(scope='module')
def g16():
    d = dict(np.load(GOLDEN / 'g16_orpit.npz', allow_pickle=False))
    d['cases'] = json.loads(str(d['cases']))
    return d


def separator(flag_units=5, num_speakers=2, mask=True, norm='gLN'):
    from padertorch_amd.contrib.examples.source_separation.tasnet import TasDecoder, TasEncoder, TasNet
    from padertorch_amd.modules import ConvNet
    return TasNet(TasEncoder(16, 12), ConvNet(input_size=8, num_blocks=2, num_repeats=1, hidden_channels=16, kernel_size=3, norm=norm),
                  TasDecoder(16, 12), mask=mask, num_speakers=num_speakers, additional_out_size=flag_units)


def model(**kw):
    from padertorch_amd.contrib.examples.source_separation.or_pit import OneAndRestPIT
    flag_units = kw.get('flag_units', 5)
    return OneAndRestPIT(separator(flag_units), **{'flag_units': flag_units, **kw})


def test_constructor_checks():
    from padertorch_amd.contrib.examples.source_separation.or_pit import OneAndRestPIT
    with pytest.raises(AssertionError, match='two outputs'):
        OneAndRestPIT(separator(5, num_speakers=3), flag_units=5)
    with pytest.raises(AssertionError, match='flag is disabled'):
        OneAndRestPIT(separator(0), flag_units=0)                                   # stop_condition defaults to 'flag'
    assert OneAndRestPIT(separator(0), flag_units=0, stop_condition='none').flag_nn is None
    with pytest.raises(ValueError, match='Unknown stopping condition'):
        model(stop_condition='never')
    with pytest.raises(ValueError, match='Unknown unroll type'):
        model(unroll_type='res-double')
    with pytest.raises(ValueError, match='Unknown flag reduction'):
        model(flag_reduction='median')
    net = model()
    assert (net.finetune, net.unroll_type, net.threshold, net.propagate_grad_between_iterations, net.flag_reduction, net.flag_units) == \
        (False, 'res-single', 0.5, False, 'mean', 5)
    assert tuple(net.flag_nn.weight.shape) == (1, 5) and tuple(net.flag_nn.bias.shape) == (1,)


def test_finalize_dogmatic_config():
    from padertorch_amd.contrib.examples.source_separation.or_pit import OneAndRestPIT
    config = dict(flag_units=7, separator=dict(num_speakers=4, additional_out_size=0))
    OneAndRestPIT.finalize_dogmatic_config(config)
    assert config['separator'] == dict(num_speakers=2, additional_out_size=7)


@pytest.mark.parametrize('reduction', ['min', 'max'])
def test_quirk_min_max_reductions_raise_at_construction(reduction):
    with pytest.raises(ValueError, match='cannot run in the reference'):
        model(flag_reduction=reduction)


def _outputs(iterations, B=2, T=16):
    return dict(outs=[dict(out=torch.zeros(B, 2, T), flag=torch.full((B,), 0.5)) for _ in range(iterations)])


def test_quirk_unequal_lengths_raise_value_error():
    net = model(unroll_type='res-silent', finetune=True)
    inputs = dict(s=torch.zeros(2, 3, 16), num_samples=[16, 12])
    with pytest.raises(ValueError, match='padded length 16'):
        net.loss(inputs, _outputs(3))
    with pytest.raises(ValueError, match='padded length 16'):
        net.review(inputs, _outputs(3))


def test_quirk_est_silent_runs_out_of_targets():
    net = model(unroll_type='est-silent', finetune=True)
    inputs = dict(s=torch.zeros(2, 3, 16), num_samples=[16, 16])
    with pytest.raises(IndexError, match='4 iterations for 3 targets'):
        net.review(inputs, _outputs(4))


def test_quirk_stop_threshold_reads_estimate():
    net = model(unroll_type='est-silent', stop_condition='threshold', threshold=0.5)
    quiet, loud = torch.full((1, 8), 0.1), torch.ones(1, 8)
    assert net.stop_condition(dict(estimate=quiet, residual=loud), 0) is True
    assert net.stop_condition(dict(estimate=loud, residual=quiet), 0) is False
    net = model(unroll_type='res-silent', stop_condition='threshold', threshold=0.5)
    assert net.stop_condition(dict(estimate=loud, residual=quiet), 0) is True
    assert model(unroll_type='res-single', stop_condition='threshold').stop_condition(dict(estimate=quiet, residual=quiet), 0) is False


def test_forward_checks_the_speaker_counts_and_flag_targets():
    net = model(finetune=True)
    with pytest.raises(AssertionError):
        net.forward(dict(y=torch.zeros(2, 16), num_samples=[16, 16], num_speakers=[2, 3]))
    assert [model(unroll_type=u)._get_flag_target(1, 3) for u in ('res-single', 'res-silent', 'est-silent')] == [True, False, False]
    assert [model(unroll_type=u)._get_flag_target(3, 3) for u in ('res-single', 'res-silent', 'est-silent')] == [False, False, True]


def test_return_mask_is_opt_in():
    from padertorch_amd.contrib.examples.source_separation.tasnet import TasNet
    assert TasNet.return_mask is False and TasNet.return_encoded_out is False


@pytest.mark.parametrize('c', 'abcdef')
def test_state_dict_keys_are_the_reference_s(g16, c):
    case = g16['cases'][c]
    from padertorch_amd.contrib.examples.source_separation.or_pit import OneAndRestPIT
    net = OneAndRestPIT(separator(case['flag_units'], mask=case['mask'], norm=case['norm']), flag_units=case['flag_units'],
                        stop_condition=case['stop_condition'])
    keys = json.loads(str(g16[c + '_keys']))
    assert list(net.state_dict()) == keys
    net.load_state_dict({k: torch.from_numpy(g16[f'{c}_p_{k}']) for k in keys}, strict=True)
    assert [n for n, _ in net.named_parameters()] == json.loads(str(g16[c + '_names']))


def test_golden_recipe_matches_the_file(g16):
    spec = importlib.util.spec_from_file_location('make_golden_orpit', GOLDEN / 'make_golden_orpit.py')
    maker = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(maker)                      # (the reference is imported by main() only)
    assert maker.CASES == g16['cases'] and list(maker.CASES) == list('abcdef')
    table = {c: (v['K'], v['unroll_type'], v['flag_reduction'], v['B']) for c, v in maker.CASES.items()}
    assert table == {'a': (2, 'res-single', 'mean', 3), 'b': (3, 'res-silent', 'res-weighted-mean', 2),
                     'c': (4, 'est-silent', 'est-weighted-mean', 2), 'd': (3, 'res-single', 'mean', 2),
                     'e': (3, 'res-single', 'mean', 2), 'f': (2, 'res-single', 'res-weighted-mean', 2)}
    assert maker.CASES['b']['propagate'] and maker.CASES['b']['norm'] == 'cLN' and maker.CASES['d']['flag_units'] == 0 \
        and maker.CASES['d']['stop_condition'] == 'none' and not maker.CASES['e']['finetune'] and not maker.CASES['f']['mask']
    for c, case in maker.CASES.items():
        y, s = maker.inputs(case, int(g16[c + '_seed']))
        assert y.shape == (case['B'], maker.T) and s.shape == (case['B'], case['K'], maker.T) and y.dtype == s.dtype == np.float32
        assert g16[c + '_out64'].shape[0] == case['B'] and g16[c + '_order'].shape[0] == case['B']
        assert float(g16[c + '_margin']) >= maker.TIE_MARGIN and float(g16[c + '_gap']) >= maker.GAP
    assert sum(k.startswith('fn_') for k in g16) == len(maker.FN_LOSSES) * 5 * 2 * 2
