#!/usr/bin/env python3
"""Generate tests/golden/g17_dprnn.npz by importing the REAL reference's DPRNN (padertorch/modules/dual_path_rnn.py) and, for the last
case, its TasNet around it.

Run in the build container only (needs /root/reference):

    python tests/golden/make_golden_dprnn.py

The reference is imported exactly as make_golden_convnet.py does.  The output is data only.  The shim's ``paderbox.array.segment_axis``
raises, so this generator patches that one function with ``segment_axis`` below (a restatement for ``axis=-2, end='pad'``) and, before
it generates anything, asserts the answers of the reference's own ``segment`` / ``overlap_add`` doctests (``dual_path_rnn.py:75-121``,
``:160-190``) through it.

DPRNN cases (input_size, rnn_size, window, hop, blocks, intra type, inter type, B, L, lengths):

    8/12/6/3/2/blstm/blstm/3/20/[20, 14, 9]    baseline, ragged
    6/5/4/3/1/lstm/blstm/2/13/[12, 12]         hop != window / 2, rnn_size 5, equal lengths shorter than L (12, not 11: the reference's
                                               intra path pads its output to max S_b chunks only and fails at the residual when no
                                               example reaches all S chunks, dual_path_rnn.py:487-497; 12 frames reach the fifth)
    8/8/auto/auto/1/blstm/lstm/1/18/None       'auto' (K = 6, P = 3), no lengths, unidirectional inter path
    8/12/6/3/1/blstm/blstm/2/20/[20, 3]        an example of little more than padding

and one ``TasNet(TasEncoder(4, 8), DPRNN(8, 12, 6, 3, 2), TasDecoder(4, 8))`` on two ragged mixtures of 62 / 41 samples (30 encoded
frames, which the DPRNN returns as 30: with frames behind the input the shorter example's output would be exactly zero there, a tie of
the PReLU behind the separator).

Lengths are in descending order: the reference's ``pack_padded_sequence`` demands it.  ``inputs(case, seed)`` draws ``x [B, L, N]`` -
random over the whole padded length, as ``TasNet``'s ``input_proj`` bias makes it in real use: the reference lets those frames into the
last valid chunk and through the residual path - and the weights ``r`` of the functional ``sum(y * r)`` from a seeded numpy RandomState;
they are NOT stored, the tests call the same function.  The norms' weights are drawn from [0.5, 1.5], their biases from [-0.5, 0.5]
(and, in the TasNet case, the PReLU slopes from [0.1, 0.4]); the TasNet case moves its seed until no ReLU / PReLU input of the fp64 run
lies within 1e-5 max|input| of zero, as make_golden_tasnet.py does.

Every case must show the reference's own fp32 run within a QUARTER of the tests' gates (values 1e-5 max|want|, gradients 2e-4
max|want|) of its fp64 run; the generator prints the shares and refuses to write the file otherwise.

Keys per case ``c<i>_``: ``keys`` / ``names`` (json lists: state_dict keys, named_parameters), ``p_<key>``, ``y64`` / ``y32`` (TasNet:
``out``), ``g64_x`` / ``g32_x`` (TasNet: w.r.t. the mixtures) and ``g64_<name>`` / ``g32_<name>`` the gradients of the functional, ``seed``;
TasNet: ``lengths`` (encoded_sequence_lengths), ``margin``.
"""
import json
import math
import sys
from pathlib import Path

HERE = Path(__file__).resolve().parent
REPO = HERE.parent.parent

import numpy as np  # noqa: E402

#: (input_size, rnn_size, window, hop, blocks, intra type, inter type, B, L, lengths)
CASES = [(8, 12, 6, 3, 2, 'blstm', 'blstm', 3, 20, [20, 14, 9]), (6, 5, 4, 3, 1, 'lstm', 'blstm', 2, 13, [12, 12]),
         (8, 8, 'auto', 'auto', 1, 'blstm', 'lstm', 1, 18, None), (8, 12, 6, 3, 1, 'blstm', 'blstm', 2, 20, [20, 3])]
TASNET = dict(L=4, N=8, rnn_size=12, window=6, hop=3, blocks=2, K=2, B=2, T=62, num_samples=[62, 41])
TIE_MARGIN = 1e-5
VALUE, GRAD = 1e-5, 2e-4
SHARE = 0.25


def geometry(case):
    """``(K, P, S, L_out)`` of a DPRNN case."""
    _, _, K, P, _, _, _, _, L, _ = case
    if K == 'auto':
        K = int(math.sqrt(2 * L))
        P = K // 2
    padded = L + 2 * (K - P)
    S = 1 if padded <= K else -(-(padded - K) // P) + 1
    return K, P, S, S * P - (K - P)


def inputs(case, seed):
    """The seeded input ``x [B, L, N]`` and the weights ``r [B, L_out, N]`` of the functional ``sum(y * r)``."""
    N, B, L = case[0], case[7], case[8]
    rng = np.random.RandomState(seed)
    return rng.randn(B, L, N).astype(np.float32), rng.randn(B, geometry(case)[3], N).astype(np.float32)


def tasnet_inputs(seed):
    """``(y [B, T], r [B, K, T])``, float32."""
    rng = np.random.RandomState(seed)
    c = TASNET
    return rng.randn(c['B'], c['T']).astype(np.float32), rng.randn(c['B'], c['K'], c['T']).astype(np.float32)


def segment_axis(x, length, shift, axis=-1, end='cut'):
    """What ``paderbox.array.segment_axis`` returns for a torch tensor with ``axis=-2, end='pad'``: windows of ``length`` every ``shift``
    along the second to last axis, the signal zero-padded at its end to a whole number of windows: ``[..., frames, length, N]``."""
    import torch
    assert axis == -2 and end == 'pad', (axis, end)
    n = x.shape[-2]
    frames = 1 if n <= length else -(-(n - length) // shift) + 1
    x = torch.nn.functional.pad(x, [0, 0, 0, (frames - 1) * shift + length - n])
    return x.unfold(-2, length, shift).transpose(-1, -2)


def check_doctests():
    """The answers of ``dual_path_rnn.py:75-121`` and ``:160-190`` through the patched ``segment_axis``."""
    import torch
    from padertorch.modules.dual_path_rnn import overlap_add, segment

    def seg(n, hop, win, length):
        s, l = segment(1 + torch.arange(n)[None, :, None], hop, win, torch.tensor(length))
        return s[0, 0].tolist(), int(l)

    full = [[0, 1, 3, 5], [0, 2, 4, 0], [1, 3, 5, 0], [2, 4, 0, 0]]
    assert seg(5, 2, 4, 5) == (full, 4)
    assert seg(5, 2, 4, 4) == (full, 3)
    assert seg(4, 2, 4, 4) == ([[0, 1, 3], [0, 2, 4], [1, 3, 0], [2, 4, 0]], 3)
    assert seg(5, 2, 4, 3) == (full, 3)
    assert seg(3, 2, 4, 3) == ([[0, 1, 3], [0, 2, 0], [1, 3, 0], [2, 0, 0]], 3)
    for hop, shape, length in ((3, (1, 1, 4, 2), 2), (1, (1, 1, 4, 8), 8)):
        s, l = segment(torch.arange(5)[None, :, None], hop, 4, torch.tensor(5))
        assert tuple(s.shape) == shape and int(l) == length, (s.shape, l)
    s, l = segment(torch.ones(1, 7912, 64), 50, 100, torch.tensor([7912]))
    assert tuple(s.shape) == (1, 64, 100, 160) and l.tolist() == [160]
    a = torch.arange(50).unsqueeze(0).unsqueeze(-1)
    added = overlap_add(segment(a, 10, 20)[0], 10, unpad=True)
    assert tuple(added.shape) == (1, 50, 1) and added[0, :, 0].tolist() == list(range(0, 100, 2))
    assert overlap_add(segment(torch.arange(5)[None, :, None], 2, 4)[0], 2)[0, :, 0].tolist() == [0, 2, 4, 6, 8, 0]
    assert overlap_add(segment(torch.arange(5)[None, :, None], 3, 4)[0], 3)[0, :, 0].tolist() == [0, 1, 4, 3, 4]


def parameter_range(name):
    """The range a parameter is redrawn from, or None to keep its initialisation."""
    leaf = name.rsplit('.', 1)[1]
    if name.startswith(('output_prelu', 'output_nonlinearity')):
        return 0.1, 0.4
    if 'norm' in name and leaf == 'weight':
        return 0.5, 1.5
    if 'norm' in name and leaf == 'bias':
        return -0.5, 0.5
    return None


def redraw(net, seed):
    import torch
    rng = np.random.RandomState(seed + 1)
    with torch.no_grad():
        for name, p in net.named_parameters():
            span = parameter_range(name)
            if span is not None:
                p.copy_(torch.from_numpy(rng.uniform(*span, size=tuple(p.shape)).astype(np.float32)))
    return net


def build(case, seed):
    import torch
    from padertorch.modules.dual_path_rnn import DPRNN  # the reference
    N, H, K, P, blocks, intra, inter, _, _, _ = case
    torch.manual_seed(seed)
    return redraw(DPRNN(N, H, K, P, blocks, inter_chunk_type=inter, intra_chunk_type=intra), seed)


def run(net, case, seed, dtype):
    import torch
    x0, r0 = inputs(case, seed)
    net = net.to(dtype)
    for p in net.parameters():
        p.grad = None
    x = torch.from_numpy(x0).to(dtype).requires_grad_()
    y = net(x, None if case[9] is None else list(case[9]))
    assert tuple(y.shape) == r0.shape, (y.shape, r0.shape)
    (y * torch.from_numpy(r0).to(dtype)).sum().backward()
    res = {'y': y.detach().numpy().copy(), 'g_x': x.grad.numpy().copy()}
    for name, p in net.named_parameters():
        res['g_' + name] = p.grad.numpy().copy()
    return res


def build_tasnet(seed):
    import torch
    from padertorch.contrib.examples.source_separation.tasnet.model import TasNet  # the reference
    from padertorch.contrib.examples.source_separation.tasnet.tas_coders import TasDecoder, TasEncoder
    from padertorch.modules.dual_path_rnn import DPRNN
    c = TASNET
    torch.manual_seed(seed)
    return redraw(TasNet(TasEncoder(c['L'], c['N']), DPRNN(c['N'], c['rnn_size'], c['window'], c['hop'], c['blocks']),
                         TasDecoder(c['L'], c['N']), num_speakers=c['K']), seed)


def run_tasnet(net, seed, dtype, margins=None):
    import torch
    y0, r0 = tasnet_inputs(seed)
    net = net.to(dtype)
    hooks = []
    if margins is not None:
        def margin_of(t):
            margins.append(float(t.detach().abs().min() / t.detach().abs().max()))
        hooks.append(net.encoder.encoder_1d.register_forward_hook(lambda _m, _args, out: margin_of(out)))
        for m in net.modules():
            if isinstance(m, (torch.nn.PReLU, torch.nn.ReLU)):
                hooks.append(m.register_forward_hook(lambda _m, args, _out: margin_of(args[0])))
    y = torch.from_numpy(y0).to(dtype).requires_grad_()
    out = net(dict(y=list(y.unbind(0)), num_samples=list(TASNET['num_samples'])))
    for h in hooks:
        h.remove()
    names = [n for n, _ in net.named_parameters()]
    grads = torch.autograd.grad((out['out'] * torch.from_numpy(r0).to(dtype)).sum(), [p for _, p in net.named_parameters()] + [y])
    res = {'y': out['out'].detach().numpy().copy(), 'lengths': np.asarray(out['encoded_sequence_lengths']).astype(np.int64)}
    for n, g in zip(names + ['x'], grads):
        res['g_' + n] = g.numpy().copy()
    return res


def shares(r32, r64):
    """{quantity: |fp32 - fp64| / (gate max|fp64|)} of the reference's two runs."""
    out = {}
    for k, want in r64.items():
        if k == 'lengths':
            continue
        gate = GRAD if k.startswith('g_') else VALUE
        out[k] = float(np.abs(r32[k].astype(np.float64) - want).max()) / (gate * float(np.abs(want).max()))
    return out


def store(out, prefix, net_params, names, r64, r32):
    out[prefix + 'keys'] = np.array(json.dumps(list(net_params)))
    out[prefix + 'names'] = np.array(json.dumps(names))
    for k, v in net_params.items():
        out[prefix + 'p_' + k] = v
    for k in r64:
        if k == 'lengths':
            out[prefix + k] = r64[k]
        elif k == 'y':
            out[prefix + 'y64'], out[prefix + 'y32'] = r64[k], r32[k]
        else:
            out[prefix + 'g64_' + k[2:]], out[prefix + 'g32_' + k[2:]] = r64[k], r32[k]


def main():
    sys.path[:0] = [str(HERE / 'ref_shim'), str(REPO), '/root/reference']
    import torch
    import paderbox

    paderbox.array.segment_axis = segment_axis
    torch.set_num_threads(1)
    torch.use_deterministic_algorithms(True)
    check_doctests()
    print('the reference\'s segment / overlap_add doctest answers hold through the patched segment_axis')
    out, worst = {}, 0.
    for i, case in enumerate(CASES):
        seed = 1700 + 100 * i
        net = build(case, seed)
        params = {k: v.numpy().copy() for k, v in net.state_dict().items()}
        names = [n for n, _ in net.named_parameters()]
        r64 = run(net, case, seed, torch.float64)
        r32 = run(build(case, seed), case, seed, torch.float32)
        sh = shares(r32, r64)
        out[f'c{i}_seed'] = np.array(seed)
        store(out, f'c{i}_', params, names, r64, r32)
        grads = [v for k, v in sh.items() if k.startswith('g_') and k != 'g_x']
        print(case, 'K P S L_out', geometry(case), 'fp32 vs fp64 relative to max|fp64|: y %.1e dx %.1e worst parameter gradient %.1e'
              % (sh['y'] * VALUE, sh['g_x'] * GRAD, max(grads) * GRAD), '= shares of the gates %.3f %.3f %.3f' % (sh['y'], sh['g_x'], max(grads)))
        worst = max(worst, max(sh.values()))
    i, seed = len(CASES), 1700 + 100 * len(CASES)
    while True:
        net = build_tasnet(seed)
        params = {k: v.numpy().copy() for k, v in net.state_dict().items()}
        names = [n for n, _ in net.named_parameters()]
        margins = []
        r64 = run_tasnet(net, seed, torch.float64, margins)
        if min(margins) >= TIE_MARGIN:
            break
        seed += 1
    r32 = run_tasnet(build_tasnet(seed), seed, torch.float32)
    sh = shares(r32, r64)
    out[f'c{i}_seed'], out[f'c{i}_margin'] = np.array(seed), np.array(min(margins))
    store(out, f'c{i}_', params, names, r64, r32)
    grads = [v for k, v in sh.items() if k.startswith('g_')]
    print('TasNet', TASNET, 'seed', seed, 'margin %.2e' % min(margins), 'fp32 vs fp64 relative to max|fp64|: out %.1e worst gradient %.1e'
          % (sh['y'] * VALUE, max(grads) * GRAD), '= shares of the gates %.3f %.3f' % (sh['y'], max(grads)))
    worst = max(worst, max(sh.values()))
    assert worst <= SHARE, f'the reference\'s fp32 run is {worst:.3f} of a gate from its fp64 run (limit {SHARE}): make the case shallower'
    out['cases'] = np.array(json.dumps(CASES))
    out['tasnet'] = np.array(json.dumps(TASNET))
    path = HERE / 'g17_dprnn.npz'
    np.savez_compressed(path, **out)
    print(path, path.stat().st_size, 'bytes')


if __name__ == '__main__':
    main()
