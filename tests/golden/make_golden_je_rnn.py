#!/usr/bin/env python3
"""Generate tests/golden/g25_je_rnn.npz by importing the REAL reference's sequence wrappers (padertorch/contrib/je/modules/rnn.py) and
poolings (contrib/je/modules/reduce.py).

Run in the build container only (needs /root/reference):

    python tests/golden/make_golden_je_rnn.py

The reference is imported exactly as make_golden_dprnn.py does.  The output is data only: parameters and the results of an fp64 and an
fp32 run of the reference.  Inputs are NOT stored: ``rnn_inputs`` / ``pool_inputs`` draw them from a seeded numpy RandomState and the
tests call the same functions.

RNN cases ``r<i>_`` on ``x [4, 10, 19]`` (``B, F, T``), lengths ``[19, 14, 9, 1]`` (descending: the reference's
``pack_padded_sequence`` demands it), functional ``sum(y * r)``:

    r0  GRU, H = 6, 2 layers, bidirectional, reverse=True, ragged
    r1  GRU, H = 5, 1 layer, unidirectional, bias=False, seq_len=None
    r2  LSTM, H = 6, 2 layers, bidirectional, ragged
    r3  TransformerEncoder: 2 layers, hidden 16, 2 heads, d_ff 32, bidirectional attention, ragged, reverse=True
    r4  RNN(GRU, H = 6, bidirectional) followed by AutoPool(12, trainable=True) as ONE functional ``sum(pool(y) * r)``

Pooling cases ``p_<module>_<l|n>_<axis>_<k>`` (lengths or none, axis -1 on ``[4, 10, 19]`` or axis 1 on ``[4, 19, 10]``, keepdims 0 / 1)
for Sum, Mean, Max (``idx``: its indices) and TakeLast; ``a_<t|f>_<l|n>`` for AutoPool(10, alpha=1.5, trainable or not) on ``[4, 10, 19]``;
``v_<l|n>`` for reverse_sequence on ``[4, 19, 10]``.  Keys per case: ``y64`` / ``y32``, ``g64_x`` / ``g32_x`` and, with parameters,
``keys`` / ``names`` (json), ``p_<key>``, ``g64_<name>`` / ``g32_<name>``.

Gradients whose fp64 run is analytically zero (max|g64| < 1e-12: the attention's key biases) have no scale to gate against; the tests
compare them against an absolute bound instead.

Every case must show the reference's own fp32 run within a QUARTER of the tests' gates (values 1e-5 max|want|, gradients 2e-4 max|want|)
of its fp64 run; the generator prints the shares and refuses to write the file otherwise.
"""
import json
import sys
from pathlib import Path

HERE = Path(__file__).resolve().parent
REPO = HERE.parent.parent

import numpy as np  # noqa: E402

B, F, T = 4, 10, 19
LENGTHS = [19, 14, 9, 1]
VALUE, GRAD = 1e-5, 2e-4
SHARE = 0.25
ZERO = 1e-12          # a gradient whose fp64 run stays below this everywhere is analytically zero: no gate applies
ALPHA = 1.5

#: name -> (kind, hidden, layers, bidirectional, bias, reverse, lengths or None)
RNN_CASES = {
    'r0': ('gru', 6, 2, True, True, True, LENGTHS),
    'r1': ('gru', 5, 1, False, False, False, None),
    'r2': ('lstm', 6, 2, True, True, False, LENGTHS),
    'r3': ('transformer', 16, 2, False, True, True, LENGTHS),
    'r4': ('gru+autopool', 6, 1, True, True, False, LENGTHS),
}
TRANSFORMER = dict(d_ff=32, num_heads=2, bidirectional=True)
POOLS = ('Sum', 'Mean', 'Max', 'TakeLast')


def out_channels(case):
    kind, H, _, bidir, _, _, _ = RNN_CASES[case]
    return H if kind == 'transformer' else H * (1 + bidir)


def rnn_inputs(case):
    """``(x [B, F, T], r)`` float32; ``r`` has the shape of the functional's operand."""
    rng = np.random.RandomState(2500 + int(case[1:]))
    C = out_channels(case)
    shape = (B, C) if RNN_CASES[case][0] == 'gru+autopool' else (B, C, T)
    return rng.randn(B, F, T).astype(np.float32), rng.randn(*shape).astype(np.float32)


def pool_cases():
    """``[(key, module name, with lengths, axis, keepdims)]``."""
    return [(f'p_{m}_{"l" if wl else "n"}_{"m1" if axis < 0 else "1"}_{int(k)}', m, wl, axis, k)
            for m in POOLS for wl in (True, False) for axis in (-1, 1) for k in (False, True)]


def pool_inputs(key, out_shape=None):
    """``x`` float32: ``[4, 10, 19]`` for axis -1, ``[4, 19, 10]`` for axis 1 (and reverse_sequence); continuous draws: no ties.  With
    ``out_shape``: ``(x, r)``."""
    rng = np.random.RandomState(abs(hash_name(key)) % (2 ** 31))
    time_last = key.startswith('a_') or (key.startswith('p_') and key.split('_')[3] == 'm1')
    x = rng.randn(*((B, F, T) if time_last else (B, T, F))).astype(np.float32)
    if out_shape is None:
        return x
    return x, rng.randn(*out_shape).astype(np.float32)


def hash_name(key):
    """A hash of the key that does not depend on the interpreter's hash seed."""
    h = 7
    for ch in key:
        h = (h * 131 + ord(ch)) % 1000003
    return h


def build_rnn(case, mods, dtype):
    import torch
    kind, H, layers, bidir, bias, reverse, _ = RNN_CASES[case]
    torch.manual_seed(2500 + int(case[1:]))
    if kind == 'transformer':
        net = mods['TransformerEncoder'](mods['TransformerLayerStack'](F, H, num_layers=layers, **TRANSFORMER), reverse=reverse)
    else:
        cls = torch.nn.LSTM if kind == 'lstm' else torch.nn.GRU
        wrap = mods['LSTM'] if kind == 'lstm' else mods['GRU']
        net = wrap(cls(F, H, layers, bias=bias, batch_first=True, bidirectional=bidir), reverse=reverse)
    pool = None
    if kind == 'gru+autopool':
        pool = mods['AutoPool'](out_channels(case), alpha=ALPHA, trainable=True)
        with torch.no_grad():
            pool.alpha.copy_(torch.linspace(0.5, 2., out_channels(case))[:, None])
    return net.to(dtype), None if pool is None else pool.to(dtype)


def run_rnn(case, mods, dtype):
    import torch
    net, pool = build_rnn(case, mods, dtype)
    x0, r0 = rnn_inputs(case)
    lengths = RNN_CASES[case][6]
    x = torch.from_numpy(x0).to(dtype).requires_grad_()
    y, _ = net(x, None if lengths is None else list(lengths))
    if pool is not None:
        y = pool(y, list(lengths))
    assert tuple(y.shape) == r0.shape, (y.shape, r0.shape)
    named = [('rnn.' + n, p) for n, p in net.named_parameters()] + ([] if pool is None else [('pool.' + n, p) for n, p in pool.named_parameters()])
    grads = torch.autograd.grad((y * torch.from_numpy(r0).to(dtype)).sum(), [x] + [p for _, p in named])
    res = {'y': y.detach().numpy().copy(), 'g_x': grads[0].numpy().copy()}
    for (n, _), g in zip(named, grads[1:]):
        res['g_' + n] = g.numpy().copy()
    state = {'rnn.' + k: v.numpy().copy() for k, v in net.state_dict().items()}
    if pool is not None:
        state.update({'pool.' + k: v.numpy().copy() for k, v in pool.state_dict().items()})
    return res, state, [n for n, _ in named]


def run_pool(key, module, with_lengths, dtype, extra=None):
    """One pooling / reverse_sequence call of the reference: ``module(x, seq_len)`` and the gradients of ``sum(y * r)``."""
    import torch
    x0 = pool_inputs(key)
    x = torch.from_numpy(x0).to(dtype).requires_grad_()
    out = module(x, list(LENGTHS) if with_lengths else None)
    res = {}
    if isinstance(out, tuple):
        res['idx'] = out[1].numpy().copy()
        out = out[0]
    _, r0 = pool_inputs(key, tuple(out.shape))
    params = [] if extra is None else [extra]
    grads = torch.autograd.grad((out * torch.from_numpy(r0).to(dtype)).sum(), [x] + params)
    res.update(y=out.detach().numpy().copy(), g_x=grads[0].numpy().copy())
    if extra is not None:
        res['g_alpha'] = grads[1].numpy().copy()
    return res


def shares(r32, r64):
    out = {}
    for k, want in r64.items():
        if k == 'idx':
            assert np.array_equal(r32[k], want), 'the reference\'s own fp32 run picks another maximum: a tie'
            continue
        gate = GRAD if k.startswith('g_') else VALUE
        if k.startswith('g_') and float(np.abs(want).max()) < ZERO:          # analytically zero (a key bias under the softmax): left out
            continue
        out[k] = float(np.abs(r32[k].astype(np.float64) - want).max()) / (gate * float(np.abs(want).max()))
    return out


def store(out, prefix, r64, r32):
    for k in r64:
        if k == 'idx':
            out[prefix + 'idx'] = r64[k]
        elif k == 'y':
            out[prefix + 'y64'], out[prefix + 'y32'] = r64[k], r32[k]
        else:
            out[prefix + 'g64_' + k[2:]], out[prefix + 'g32_' + k[2:]] = r64[k], r32[k]


def main():
    sys.path[:0] = [str(HERE / 'ref_shim'), str(REPO), '/root/reference']
    import torch
    from padertorch.contrib.je.modules import reduce as ref_reduce  # the reference
    from padertorch.contrib.je.modules import rnn as ref_rnn
    from padertorch.contrib.je.modules.transformer import TransformerLayerStack

    torch.set_num_threads(1)
    torch.use_deterministic_algorithms(True)
    mods = {n: getattr(ref_rnn, n) for n in ('GRU', 'LSTM', 'TransformerEncoder')}
    mods.update(TransformerLayerStack=TransformerLayerStack, AutoPool=ref_reduce.AutoPool)
    out, worst = {}, 0.
    for case in RNN_CASES:
        r64, state, names = run_rnn(case, mods, torch.float64)
        r32, state32, _ = run_rnn(case, mods, torch.float32)
        sh = shares(r32, r64)
        out[case + '_keys'] = np.array(json.dumps(list(state32)))
        out[case + '_names'] = np.array(json.dumps(names))
        for k, v in state32.items():
            out[case + '_p_' + k] = v
        store(out, case + '_', r64, r32)
        print(case, RNN_CASES[case], 'shares of the gates: y %.3f dx %.3f worst parameter gradient %.3f'
              % (sh['y'], sh['g_x'], max(v for k, v in sh.items() if k not in ('y', 'g_x'))))
        worst = max(worst, max(sh.values()))
    for key, name, wl, axis, keep in pool_cases():
        module = getattr(ref_reduce, name)(axis=axis, keepdims=keep)
        r64, r32 = run_pool(key, module, wl, torch.float64), run_pool(key, module, wl, torch.float32)
        sh = shares(r32, r64)
        store(out, key + '_', r64, r32)
        print(key, 'shares of the gates: ' + ' '.join('%s %.3f' % kv for kv in sh.items()))
        worst = max(worst, max(sh.values()))
    for trainable in (True, False):
        for wl in (True, False):
            key = f'a_{"t" if trainable else "f"}_{"l" if wl else "n"}'
            res = []
            for dtype in (torch.float64, torch.float32):
                pool = ref_reduce.AutoPool(F, alpha=ALPHA, trainable=trainable).to(dtype)
                res.append(run_pool(key, pool, wl, dtype, pool.alpha if trainable else None))
            sh = shares(res[1], res[0])
            store(out, key + '_', res[0], res[1])
            print(key, 'shares of the gates: ' + ' '.join('%s %.3f' % kv for kv in sh.items()))
            worst = max(worst, max(sh.values()))
    for wl in (True, False):
        key = f'v_{"l" if wl else "n"}'
        r64, r32 = (run_pool(key, ref_rnn.reverse_sequence, wl, dt) for dt in (torch.float64, torch.float32))
        sh = shares(r32, r64)
        store(out, key + '_', r64, r32)
        print(key, 'shares of the gates: ' + ' '.join('%s %.3f' % kv for kv in sh.items()))
        worst = max(worst, max(sh.values()))
    assert worst <= SHARE, f'the reference\'s fp32 run is {worst:.3f} of a gate from its fp64 run (limit {SHARE}): make the case shallower'
    out['rnn_cases'] = np.array(json.dumps(RNN_CASES))
    out['lengths'] = np.array(LENGTHS)
    path = HERE / 'g25_je_rnn.npz'
    np.savez_compressed(path, **out)
    print(path, path.stat().st_size, 'bytes; worst share %.3f' % worst)


if __name__ == '__main__':
    main()
