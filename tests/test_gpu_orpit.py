"""OneAndRestPIT on the HIP path against the reference's fp64 results (tests/golden/g16_orpit.npz, made by
tests/golden/make_golden_orpit.py from the real reference).

Gates (the project's own, tests/test_gpu_tasnet.py:37): values |diff| <= 1e-5 max|want|, gradients |diff| <= 2e-4 max|want|, the loss
scalars within 1e-4, the chosen target order exactly.  The recipe refuses a seed on which the reference's own fp32 run is further than
half of these from its fp64 run, or on which two candidate targets are closer than 1e-3.  Every comparison prints its ratio (-s)."""
import importlib.util
import json
from pathlib import Path

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

GOLDEN = Path(__file__).resolve().parent / 'golden'
VALUE, GRAD, SCALAR = 1e-5, 2e-4, 1e-4
CASES = 'abcdef'


@pytest.fixture(scope='module')
def g16():
    d = dict(np.load(GOLDEN / 'g16_orpit.npz', allow_pickle=False))
    d['cases'] = json.loads(str(d['cases']))
    spec = importlib.util.spec_from_file_location('make_golden_orpit', GOLDEN / 'make_golden_orpit.py')
    d['maker'] = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(d['maker'])             # for inputs(): the seeded signals (the reference is not imported)
    return d


def close(name, got, want, gate):
    got = got.detach().double().cpu().reshape(-1)
    want = torch.as_tensor(np.asarray(want)).double().reshape(-1)
    assert got.shape == want.shape, (name, got.shape, want.shape)
    err, bound = float((got - want).abs().max()), gate * float(want.abs().max())
    ratio = err / bound if bound > 0 else (0. if err == 0 else float('inf'))
    print(f'orpit ratio {name}: {ratio:.4f} of the gate {gate:g}')
    assert ratio <= 1.0, (name, ratio)
    return ratio


def build_model(g16, c):
    from padertorch_amd.contrib.examples.source_separation.or_pit import OneAndRestPIT
    from padertorch_amd.contrib.examples.source_separation.tasnet import TasDecoder, TasEncoder, TasNet
    from padertorch_amd.modules import ConvNet
    case = g16['cases'][c]
    separator = TasNet(TasEncoder(16, 12), ConvNet(input_size=8, num_blocks=2, num_repeats=1, hidden_channels=16, kernel_size=3,
                                                   norm=case['norm']),
                       TasDecoder(16, 12), mask=case['mask'], num_speakers=2, additional_out_size=case['flag_units'])
    net = OneAndRestPIT(separator, finetune=case['finetune'], unroll_type=case['unroll_type'], stop_condition=case['stop_condition'],
                        propagate_grad_between_iterations=case['propagate'], flag_reduction=case['flag_reduction'],
                        flag_units=case['flag_units'])
    p = c + '_'
    net.load_state_dict({k: torch.from_numpy(g16[p + 'p_' + k]) for k in json.loads(str(g16[p + 'keys']))}, strict=True)
    return net.cuda(), case, p


def batch_of(g16, case, seed):
    y, s = (torch.from_numpy(a).cuda() for a in g16['maker'].inputs(case, seed))
    T = y.shape[1]
    return dict(y=y, s=s, num_samples=[T] * case['B'], num_speakers=[case['K']] * case['B'])


@pytest.mark.parametrize('c', CASES)
def test_model_matches_the_reference_fp64(g16, c):
    net, case, p = build_model(g16, c)
    names = json.loads(str(g16[p + 'names']))
    params = dict(net.named_parameters())
    assert list(params) == names and list(net.state_dict()) == json.loads(str(g16[p + 'keys']))
    batch = batch_of(g16, case, int(g16[p + 'seed']))
    out = net(batch)
    order = g16[p + 'order']
    assert len(out['outs']) == order.shape[1] and out['out'].shape == g16[p + 'out64'].shape
    assert 'encoded_out' not in out['outs'][0] and 'mask' not in out['outs'][0]
    close(f'{c} out', out['out'], g16[p + 'out64'], VALUE)
    for k, o in enumerate(out['outs']):
        close(f'{c} iteration {k} out', o['out'], g16[p + f'it{k}_out64'], VALUE)
        assert torch.equal(o['estimate'], o['out'][:, 0]) and torch.equal(o['residual'], o['out'][:, 1])
        if case['flag_units']:
            assert o['pre_mean_flag'].shape == g16[p + f'it{k}_pre64'].shape
            close(f'{c} iteration {k} flag', o['flag'], g16[p + f'it{k}_flag64'], VALUE)
            close(f'{c} iteration {k} pre_mean_flag', o['pre_mean_flag'], g16[p + f'it{k}_pre64'], VALUE)
        else:
            assert 'flag' not in o and 'pre_mean_flag' not in o
    review = net.review(batch, out)
    assert sorted(review) == sorted(json.loads(str(g16[p + 'review_keys'])))
    scalar_names = json.loads(str(g16[p + 'scalar_names']))
    assert list(review['scalars']) + ['loss'] == scalar_names
    got = torch.stack([review['scalars'][k].detach().float().reshape(()) for k in scalar_names[:-1]] + [review['loss'].detach()])
    worst = float((got.double().cpu() - torch.from_numpy(g16[p + 'scalars64'])).abs().max())
    print(f'orpit {c} scalars: worst difference {worst:.2e} (gate {SCALAR:g})')
    assert worst <= SCALAR
    assert set(review['audios']) == {f'estimate/{case["K"]}spk', f'residual-estimate/{case["K"]}spk'}
    assert net.loss(batch, out)['permutations'].t().tolist() == order.tolist()                  # the chosen target order, exactly
    grads = torch.autograd.grad(review['loss'], [params[n] for n in names])
    worst = max(close(f'{c} d {n}', g, g16[p + 'g64_' + n], GRAD) for n, g in zip(names, grads))
    print(f'orpit ratio {c} worst gradient: {worst:.4f}')


@pytest.mark.parametrize('c', CASES)
def test_decode_counts_like_the_reference(g16, c):
    net, case, p = build_model(g16, c)
    batch = batch_of(g16, case, int(g16[p + 'seed']))
    with torch.no_grad():
        out = net.decode(dict(y=batch['y'][:1], num_samples=batch['num_samples'][:1]), max_iterations=4)
    assert len(out['outs']) == int(g16[p + 'decode_iterations'])
    expected = len(out['outs']) + {'res-single': 1, 'res-silent': 0, 'est-silent': -1}[case['unroll_type']]
    assert out['out'].shape == (1, expected, batch['y'].shape[1]) and out['out'].is_cuda


def test_encoded_keys_on_request(g16):
    net, case, p = build_model(g16, 'b')
    batch = batch_of(g16, case, int(g16[p + 'seed']))
    plain = net(batch)
    net.return_encoded = True
    out = net(batch)
    assert torch.equal(out['out'], plain['out'])
    o = out['outs'][0]
    assert o['encoded_out'].shape[:2] == (case['B'], 2) and torch.equal(o['encoded_estimate'], o['encoded_out'][:, 0]) \
        and torch.equal(o['encoded_residual'], o['encoded_out'][:, 1])


def _step(net, batch):
    """forward + loss + backward: [loss, reconstruction loss, the chosen targets, d parameters...]."""
    out = net(batch)
    losses = net.loss(batch, out)
    grads = torch.autograd.grad(losses['loss'], list(net.parameters()))
    return [losses['loss'].detach(), losses['reconstruction_loss'].detach(), losses['permutations']] + list(grads)


def test_step_is_capturable_and_the_target_choice_is_device_data(g16):
    """Case b's forward + loss + backward captured once and replayed on two batches whose golden target orders differ: each replay is
    bit-identical to the eager step on the same batch."""
    from padertorch_amd.ops import capture
    net, case, p = build_model(g16, 'b')
    first = batch_of(g16, case, int(g16[p + 'seed']))
    second = batch_of(g16, case, int(g16['b_alt_seed']))
    assert g16['b_order'].tolist() != g16['b_alt_order'].tolist()
    lengths = torch.tensor(first['num_samples'], device='cuda')
    static = dict(y=first['y'].clone(), s=first['s'].clone(), num_samples=lengths, num_speakers=first['num_speakers'])
    eager_first, eager_second = _step(net, dict(first, num_samples=lengths)), _step(net, dict(second, num_samples=lengths))
    for a, b in zip(eager_first, _step(net, dict(first, num_samples=lengths))):
        assert torch.equal(a, b)                                                              # two runs are bit-identical
    assert eager_first[2].t().tolist() == g16['b_order'].tolist() and eager_second[2].t().tolist() == g16['b_alt_order'].tolist()
    assert abs(float(eager_second[0]) - float(g16['b_alt_loss64'][0])) <= SCALAR
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        _step(net, static)                                                                    # eager warm-up on the capture stream
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with capture.capture_mode():
        with torch.cuda.graph(graph, stream=side):
            capture.zero_block(static['y'].device)
            captured = _step(net, static)
    graph.replay()
    torch.cuda.synchronize()
    for i, (a, b) in enumerate(zip(captured, eager_first)):
        assert torch.equal(a, b), ('replay', i)
    static['y'].copy_(second['y'])
    static['s'].copy_(second['s'])
    graph.replay()
    torch.cuda.synchronize()
    for i, (a, b) in enumerate(zip(captured, eager_second)):
        assert torch.equal(a, b), ('replay on the second batch', i)


@pytest.mark.parametrize('name', ['log_mse_loss', 'mse_loss'])
def test_loss_function_matches_the_reference(g16, name):
    from padertorch_amd.ops import losses
    fn = getattr(losses, name)
    for K in range(5):
        for length in (1, 57):
            for fill in (False, True):
                x, t = (torch.from_numpy(a).cuda() for a in g16['maker'].fn_inputs(K, length))
                loss, perm = losses.one_and_rest_permutation_invariant_loss(x, t, fn, fill_missing_with_zeros=fill)
                want_loss, want_perm = g16[f'fn_{name}_K{K}_T{length}_{int(fill)}']
                assert int(perm) == int(want_perm), (K, length, fill)
                assert abs(float(loss) - want_loss) <= VALUE * max(1., abs(want_loss)), (K, length, fill, float(loss), want_loss)
    x = torch.from_numpy(g16['maker'].fn_inputs(3, 57)[0]).cuda().requires_grad_()
    t = torch.from_numpy(g16['maker'].fn_inputs(3, 57)[1]).cuda()
    loss, perm = losses.one_and_rest_permutation_invariant_loss(x, t, fn, fill_missing_with_zeros=True)
    x64, t64 = x.detach().double().cpu().requires_grad_(), t.double().cpu()
    rest = t64[[j for j in range(3) if j != int(perm)]].sum(0)
    f64 = (lambda a, b: torch.log10(((a - b) ** 2).mean())) if name == 'log_mse_loss' else (lambda a, b: ((a - b) ** 2).mean())
    want = torch.autograd.grad(f64(x64[0], t64[int(perm)]) + f64(x64[1], rest) / 2, x64)[0]
    close(f'{name} d inputs', torch.autograd.grad(loss, x)[0], want, GRAD)
