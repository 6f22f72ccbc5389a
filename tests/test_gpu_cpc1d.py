"""``contrib.mk.modules.contrastive.CPC1d`` against the record of the reference's own ``CPC1d`` run in fp64 on the CPU
(``tests/golden/g30_cpc.npz``, ``make_golden_cpc.py``): strict ``state_dict`` load, loss, review scalars, dense logits and the encoder's
parameter gradients.

Gates: four times the reference's own fp32-vs-fp64 difference per quantity (stored by the generator), the largest over the three
configurations, relative to the quantity's largest fp64 magnitude.  Where that difference is below what fp32 can express - the review
scalars differ by exactly 0, the mean loss by 2e-9 in one configuration - the fp32 spacing 2^-23 is added: the values pass through fp32."""
import importlib.util
import json
from pathlib import Path

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

_spec = importlib.util.spec_from_file_location('make_golden_cpc', Path(__file__).parent / 'golden' / 'make_golden_cpc.py')
_gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(_gen)
CASES, build = _gen.CASES, _gen.build
GOLDEN = np.load(Path(__file__).parent / 'golden' / 'g30_cpc.npz')
D32 = np.max([GOLDEN[f'{c}_d32'] for c in CASES], axis=0)
GATES = dict(zip(('ce', 'scalars', 'logits', 'gradients'), 4 * D32 + 2. ** -23))


def model_of(case, **extra):
    from padertorch_amd.contrib.je.modules.conv import CNN1d
    from padertorch_amd.contrib.mk.modules.contrastive import CPC1d
    return build(CPC1d, CNN1d, case, torch.float32, **extra)


@pytest.mark.parametrize('case', sorted(CASES))
def test_against_reference_record(case):
    model = model_of(case, dense_logits=True)
    state = {k: torch.from_numpy(GOLDEN[f'{case}_p_{k}']).float() for k in json.loads(str(GOLDEN['keys']))}
    model.load_state_dict(state, strict=True)
    model.cuda()
    batch = dict(x=torch.from_numpy(GOLDEN['x']).cuda(), seq_len=GOLDEN['seq_len'].tolist(), labels=GOLDEN['labels'])
    outputs = model(batch)
    review = model.review(batch, outputs)
    ce = review['losses']['ce']
    named = [(n, p) for n, p in model.named_parameters() if n.startswith('encoder.')]
    grads = torch.autograd.grad(ce, [p for _, p in named])
    errors = {'ce': abs(float(ce) - float(GOLDEN[f'{case}_ce'])) / abs(float(GOLDEN[f'{case}_ce'])), 'scalars': 0., 'logits': 0., 'gradients': 0.}
    names = json.loads(str(GOLDEN[f'{case}_scalar_names']))
    assert list(review['scalars']) == names
    for k, want in zip(names, GOLDEN[f'{case}_scalars']):
        errors['scalars'] = max(errors['scalars'], abs(float(review['scalars'][k]) - want) / abs(want))
    want_logits = [GOLDEN[f'{case}_logits{i}'] for i in range(len(outputs[0]))]
    top = max(np.abs(w[np.isfinite(w)]).max() for w in want_logits)
    for st, want in zip(outputs[0], want_logits):
        got, fin = st.logits.cpu().double().numpy(), np.isfinite(want)
        assert got.shape == want.shape and np.array_equal(np.isfinite(got), fin)
        errors['logits'] = max(errors['logits'], np.abs(got[fin] - want[fin]).max() / top)
    for (n, _), g in zip(named, grads):
        want = GOLDEN[f'{case}_g_{n}']
        errors['gradients'] = max(errors['gradients'], np.abs(g.cpu().double().numpy() - want).max() / np.abs(want).max())
    print(case, errors, GATES)
    for k in GATES:
        assert errors[k] <= GATES[k], (k, errors, GATES)
    assert model.get_posteriors(outputs).shape == (3,)


def test_unsupported_requests_raise():
    with pytest.raises(NotImplementedError, match='cosine'):
        model_of('time', similarity='cosine')
    from padertorch_amd.ops.cpc_contrast import contrastive_scores, max_features
    d = max_features() + 1
    with pytest.raises(NotImplementedError, match='ptmi_cpc_max_features'):
        contrastive_scores(torch.zeros(1, d, 4, device='cuda'), torch.zeros(1, d, 4, device='cuda'), (1,), 'time')
