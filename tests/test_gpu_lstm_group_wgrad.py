"""A BLSTM layer's weight gradients through the grouped call (``ops.lstm.GROUP_WGRAD``: one pack launch and one GEMM launch for both
directions' dW_ih and dW_hh) against the separate calls it replaces, against fp64 ``torch.nn.LSTM``, and inside a captured step."""
import copy

import numpy as np
import pytest
import torch
from torch.nn.utils.rnn import pack_sequence

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
H, B, T = 40, 5, 9


def _layer_grads(ref, xs, w, group, prefill, x_grad, monkeypatch):
    """Parameter gradients of one BLSTM layer on the Trainer's path (in place, weight-gradient queue) and the timer names of its launches."""
    from padertorch_amd import _lib
    from padertorch_amd.ops import lstm as L
    from padertorch_amd.ops import packed_lstm
    monkeypatch.setattr(L, 'DEFER_WGRAD', True)
    monkeypatch.setattr(L, 'GROUP_WGRAD', group)
    net = copy.deepcopy(ref).float().to(DEV)
    g = torch.Generator(device=DEV).manual_seed(11)
    for p in net.parameters():
        p.grad = torch.randn(p.shape, device=DEV, generator=g) if prefill else torch.zeros_like(p)
    start = {k: p.grad.clone() for k, p in net.named_parameters()}
    xg = [x.float().to(DEV).requires_grad_(x_grad) for x in xs]
    monkeypatch.setattr(_lib, 'KERNEL_TIMERS', [])
    y = packed_lstm(net, pack_sequence(xg))
    (y.data * pack_sequence([v.float().to(DEV) for v in w]).data).sum().backward()
    L.sync_deferred()
    torch.cuda.synchronize()
    L.check_errors()
    names = [n for n, _, _ in _lib.KERNEL_TIMERS]
    monkeypatch.setattr(_lib, 'KERNEL_TIMERS', None)
    return {k: (p.grad - start[k]).cpu() for k, p in net.named_parameters()}, names


@pytest.mark.parametrize('x_grad', [False, True], ids=['bottom', 'upper'])         # the step's tail (main queue) / beside a recurrence (side queue)
@pytest.mark.parametrize('prefill', [False, True])
@pytest.mark.parametrize('lens', [[T] * B, [9, 8, 6, 6, 2], [T] * 16], ids=['equal', 'ragged', 'equal16'])
@pytest.mark.parametrize('I', [24, 2 * H])
def test_grouped_weight_gradients_equal_the_separate_calls(I, lens, prefill, x_grad, monkeypatch):
    torch.manual_seed(I + len(set(lens)))
    ref = torch.nn.LSTM(I, H, 1, bidirectional=True).double()
    xs = [torch.randn(n, I, dtype=torch.float64) for n in lens]
    w = [torch.randn(n, 2 * H, dtype=torch.float64) for n in lens]
    out = ref(pack_sequence(xs))[0]
    (out.data * pack_sequence(w).data).sum().backward()
    want = {k: p.grad.clone() for k, p in ref.named_parameters()}
    on, names_on = _layer_grads(ref, xs, w, True, prefill, x_grad, monkeypatch)
    off, names_off = _layer_grads(ref, xs, w, False, prefill, x_grad, monkeypatch)
    assert not any(n.startswith(('gemm_group_bf16:', 'pack_planes_bf16_list:')) for n in names_off)
    # the separate calls' launches: bf16 GEMMs with M = 4H or 8H rows (the input gradient's has M = packed rows) and the packs of their operands
    rows = sum(lens)
    separate = (f'gemm_planes_bf16:{4 * H}x', f'gemm_planes_bf16:{8 * H}x', f'pack_planes_bf16:{rows}x')
    if any(n.startswith(separate[:2]) for n in names_off):
        # they ran on the recurrence's bf16 planes: the grouped call replaces all of them by one pack and one GEMM launch
        assert sum(n.startswith('gemm_group_bf16:') for n in names_on) == 1 and sum(n.startswith('pack_planes_bf16_list:') for n in names_on) == 1
        assert not any(n.startswith(separate) for n in names_on), names_on
    if len(lens) == 16:
        # (the recurrence hands dgates^T on as planes for equal lengths in whole 16-row tiles: B = 5 checks that every other path is
        #  what it was, B = 16 is the smallest batch the grouped call runs at)
        assert any(n.startswith('gemm_group_bf16:') for n in names_on), names_on
    assert set(on) == set(off) == set(want) and len(on) == 8
    for k in on:
        big = float(off[k].abs().max())
        d = float((on[k] - off[k]).abs().max())
        print(f'{k}: |on - off| = {d:.3g}, largest entry {big:.3g}')
        assert d <= 1e-6 * big, (k, d, big)
        # the gate tests/test_gpu_lstm.py::test_packed_lstm_vs_torch_cpu applies to parameter gradients, against fp64 torch.nn.LSTM
        scale = max(1., float(want[k].abs().max()))
        np.testing.assert_allclose(on[k].double().numpy(), want[k].numpy(), atol=3e-5 * scale, err_msg=k)


def test_grouped_weight_gradients_inside_a_captured_step(tmp_path, monkeypatch):
    """``Trainer(graph_steps=True)`` on a toy PIT model (as tests/test_gpu_graphed.py builds it) with the grouped call in the captured
    step: the replays leave the parameters of the eager loop of the same build."""
    import padertorch_amd as pt
    from padertorch_amd.contrib.examples.source_separation.pit.model import PermutationInvariantTrainingModel
    from padertorch_amd.ops import lstm as L
    from padertorch_amd.ops import pit_features
    assert L.GROUP_WGRAD
    taken = []
    grouped = L._WgradJob._grouped
    monkeypatch.setattr(L._WgradJob, '_grouped', lambda self, dg_t, ranges: taken.append(grouped(self, dg_t, ranges)) or taken[-1])
    g = torch.Generator().manual_seed(0)
    exs = []
    for _ in range(12):
        s = 0.1 * torch.randn(16, 2, 6000, generator=g)          # (16 examples: the smallest batch whose recurrence hands planes on)
        f = pit_features(s.sum(1).to(DEV), s.to(DEV))
        exs.append({k: (list(v) if isinstance(v, list) else v) for k, v in f.items()})
    torch.cuda.synchronize()
    lw = dict(pit_ips_loss=1., pit_mse_loss=0.)

    def train(path, **kw):
        torch.manual_seed(0)
        model = PermutationInvariantTrainingModel(F=257, recurrent_layers=2, units=32, K=2)
        t = pt.Trainer(model, path, pt.optimizer.Adam(gradient_clipping=1.), loss_weights=lw, summary_trigger=(1, 'iteration'),
                       checkpoint_trigger=(1000, 'iteration'), stop_trigger=(6, 'iteration'), virtual_minibatch_size=2,
                       deferred_checks=True, **kw)
        t.train(exs, device=DEV)
        return model, t
    a, ta = train(tmp_path / 'a')
    n_eager = sum(taken)
    b, tb = train(tmp_path / 'b', graph_steps=True)
    assert ta.iteration == tb.iteration == 6
    assert n_eager > 0 and sum(taken) > n_eager, taken          # the grouped call ran in the eager loop and while capturing
    for (k, v), (_, u) in zip(a.state_dict().items(), b.state_dict().items()):
        np.testing.assert_allclose(u.cpu().numpy(), v.cpu().numpy(), rtol=0, atol=1e-6, err_msg=k)
