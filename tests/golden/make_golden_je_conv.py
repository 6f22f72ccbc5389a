#!/usr/bin/env python3
"""Generate tests/golden/g26_je_conv.npz by importing the REAL reference's convolution stack (padertorch/contrib/je/modules/conv.py,
conv_utils.py).

Run in the build container only (needs /root/reference):

    python tests/golden/make_golden_je_conv.py

The reference is imported exactly as make_golden_je_rnn.py does.  The output is data only: parameters and the results of an fp64 and an
fp32 run of the reference.  Inputs are NOT stored: ``inputs`` / ``pool_inputs`` draw them from a seeded numpy RandomState and the tests
call the same functions.

All cases run on ``x [3, 6, 23]`` with lengths ``[23, 17, 9]`` (random values behind the lengths too), functional ``sum(y * r)``; biases,
``gamma``, ``beta`` and PReLU slopes carry a seeded perturbation of 0.3 N(0, 1).  ``CASES`` lists the constructors.  Keys per case:
``y64`` / ``y32``, ``g64_x`` / ``g32_x``, ``len`` (the returned lengths), ``keys`` / ``names`` (json), ``p_<key>``, ``g64_<name>`` /
``g32_<name>``; for the stacks ``shapes``, ``seqlens`` (the per-layer lists of ``get_shapes`` / ``get_sequence_lengths``), ``rf``
(``get_receptive_field``) and ``idx<i>`` (pool indices of layer ``i``).  ``n0e_``: an
evaluation pass of ``n0`` after two training passes (``y64``, ``b_<buffer>``).  ``q_<pad>_``: ``Pool1d('max', 3, 2, pad)`` on ``[2, 3, 11]``
with lengths ``[11, 6]`` (``y64``, ``idx``, ``g64_x``, ``len``).

Gates of the tests: values 1e-5 max|want|, gradients 2e-4 max|want|.  The gradient of a convolution bias that a normalisation directly
follows is zero in exact arithmetic (fp64: 1e-15, fp32: 1e-6): such a gradient (``ZERO_BIAS``: below 1e-9 of its convolution's weight
gradient in the fp64 run) is scaled by max|want| of that weight gradient.  The reference's own fp32 run must stay within a QUARTER of
every gate; the generator prints the shares and refuses to write the file otherwise.  No max-pool window of the ``q_`` cases may hold a tie.
"""
import json
import sys
from pathlib import Path

HERE = Path(__file__).resolve().parent
REPO = HERE.parent.parent

import numpy as np  # noqa: E402

B, C, T = 3, 6, 23
LENGTHS = [23, 17, 9]
VALUE, GRAD = 1e-5, 2e-4
SHARE = 0.25
ZERO_BIAS = 1e-9
POOL_SHAPE, POOL_LENGTHS = (2, 3, 11), [11, 6]
POOL_PADS = ('both', 'front', 'end', None)

#: name -> (class name, positional arguments, keyword arguments)
CASES = {
    'c0': ('Conv1d', (6, 10, 3), {}),
    'c1': ('Conv1d', (6, 10, 5), dict(stride=2, dilation=2, pad_type='front', norm='batch', activation_fn='leaky_relu', gated=True)),
    'c2': ('Conv1d', (6, 10, 4), dict(pad_type=None, norm='sequence', activation_fn='elu', pre_activation=True)),
    'c3': ('Conv1d', (6, 7, 3), dict(stride=3, pad_type='end', activation_fn='tanh', bias=False)),
    'c4': ('Conv1d', (6, 9, 1), dict(pad_type=None, activation_fn='prelu')),
    'n0': ('CNN1d', (6, [12, 12, 12, 5], 3), dict(norm='batch', residual_connections=[None, 3, None, None], pool_size=[1, 2, 1, 1],
                                                  gated=True, return_pool_indices=True)),
    'n1': ('CNN1d', (6, [8, 8, 4], [3, 5, 1]), dict(dense_connections=[None, 2, None], pre_activation=True, norm='sequence',
                                                    pool_type='avg', pool_size=[2, 1, 1], stride=[1, 2, 1], input_layer=False,
                                                    output_layer=False)),
    'n2': ('CNN1d', (6, [10, 14, 3], 3), dict(residual_connections=[2, None, None], dilation=[1, 2, 4], pad_type='front',
                                              normalize_skip_convs=True, norm='batch')),
}


def seed_of(case):
    return 2600 + sorted(CASES).index(case)


def inputs(case, out_shape=None):
    """``x [B, C, T]`` float32 and, with ``out_shape``, ``r``."""
    rng = np.random.RandomState(seed_of(case))
    x = rng.randn(B, C, T).astype(np.float32)
    return x if out_shape is None else (x, rng.randn(*out_shape).astype(np.float32))


def pad_size(size, stride, pad):
    """``(front, end)`` zeros around a pool of ``size`` every ``stride`` (the reference's ``compute_pad_size`` at dilation 1; ``main``
    checks it against the reference)."""
    overlap, rest = max(size - stride, 0), min(stride - 1, size - 1)
    return {None: (0, 0), 'front': (overlap, rest), 'both': (overlap // 2, rest + (overlap + 1) // 2), 'end': (0, size - 1)}[pad]


def pool_inputs(pad, out_shape=None):
    rng = np.random.RandomState(2650 + POOL_PADS.index(pad))
    front, end = pad_size(3, 2, pad)
    while True:                 # redrawn from the same stream until no window ties (two zeros of the padding beat a negative value)
        x = rng.randn(*POOL_SHAPE).astype(np.float32)
        if unique_maximum(x, (POOL_SHAPE[2] + front + end - 3) // 2 + 1, 3, 2, front, end).all():
            break
    return x if out_shape is None else (x, rng.randn(*out_shape).astype(np.float32))


def build(case, mods, dtype):
    """The module of ``case`` from the classes ``mods`` with seeded, perturbed parameters."""
    import torch
    cls, args, kwargs = CASES[case]
    torch.manual_seed(seed_of(case))
    net = mods[cls](*args, **kwargs)
    rng = np.random.RandomState(100 + seed_of(case))
    with torch.no_grad():
        for name, p in net.named_parameters():
            if name.endswith(('bias', 'gamma', 'beta', 'activation_fn.weight')):
                p.add_(torch.from_numpy(0.3 * rng.randn(*p.shape)).to(p.dtype))
    return net.to(dtype)


def run(case, mods, dtype, net=None):
    import torch
    net = build(case, mods, dtype) if net is None else net
    x = torch.from_numpy(inputs(case)).to(dtype).requires_grad_()
    out = net(x, list(LENGTHS))
    y = out[0]
    _, r0 = inputs(case, tuple(y.shape))
    named = list(net.named_parameters())
    grads = torch.autograd.grad((y * torch.from_numpy(r0).to(dtype)).sum(), [x] + [p for _, p in named])
    res = {'y': y.detach().numpy().copy(), 'g_x': grads[0].numpy().copy(), 'len': np.asarray(out[1])}
    for (n, _), g in zip(named, grads[1:]):
        res['g_' + n] = g.numpy().copy()
    if len(out) > 2:
        for i, idx in enumerate(out[2]):
            if idx is not None:
                res[f'idx{i}'] = idx.numpy().copy()
    return res, net


def shares(r32, r64):
    out = {}
    for k, want in r64.items():
        if k == 'len' or k.startswith('idx'):
            continue
        gate = GRAD if k.startswith('g_') else VALUE
        scale = float(np.abs(want).max())
        if k.endswith('conv.bias'):
            wscale = float(np.abs(r64[k[:-4] + 'weight']).max())
            if scale < ZERO_BIAS * wscale:
                scale = wscale
        out[k] = float(np.abs(r32[k].astype(np.float64) - want).max()) / (gate * scale)
    return out


def store(out, prefix, r64, r32):
    for k in r64:
        if k == 'len' or k.startswith('idx'):
            out[prefix + k] = r64[k]
        elif k == 'y':
            out[prefix + 'y64'], out[prefix + 'y32'] = r64[k], r32[k]
        else:
            out[prefix + 'g64_' + k[2:]], out[prefix + 'g32_' + k[2:]] = r64[k], r32[k]


def unique_maximum(x, windows, size, stride, front, end):
    """Per window (``windows`` of them on the padded axis of ``x [B, C, T]``): the maximum occurs once."""
    xp = np.pad(x, ((0, 0), (0, 0), (front, end)))
    win = np.stack([xp[..., j * stride:j * stride + size] for j in range(windows)], axis=2)
    return (win == win.max(-1, keepdims=True)).sum(-1) == 1


def main():
    sys.path[:0] = [str(HERE / 'ref_shim'), str(REPO), '/root/reference']
    if not hasattr(np, 'int'):
        np.int = int                    # the reference's get_receptive_field still says np.int
    import torch
    from padertorch.contrib.je.modules import conv as ref_conv  # the reference
    from padertorch.contrib.je.modules import conv_utils as ref_utils

    torch.set_num_threads(1)
    torch.use_deterministic_algorithms(True)
    mods = {'Conv1d': ref_conv.Conv1d, 'CNN1d': ref_conv.CNN1d}
    out, worst = {}, 0.
    for case in CASES:
        r64, net64 = run(case, mods, torch.float64)
        r32, net32 = run(case, mods, torch.float32)
        sh = shares(r32, r64)
        names = [n for n, _ in net32.named_parameters()]
        state = build(case, mods, torch.float32).state_dict()
        out[case + '_keys'] = np.array(json.dumps(list(state)))
        out[case + '_names'] = np.array(json.dumps(names))
        for k, v in state.items():
            out[f'{case}_p_{k}'] = v.numpy().copy()
        store(out, case + '_', r64, r32)
        if case.startswith('n'):
            out[case + '_shapes'] = np.array(json.dumps([[int(v) for v in s] for s in net64.get_shapes(input_shape=(B, C, T))]))
            seqlens = [np.asarray(LENGTHS)]
            for i, conv in enumerate(net64.convs):                  # (the reference's get_sequence_lengths calls a method without its
                cur = conv.get_output_sequence_lengths(seqlens[-1], None)     # ``state`` argument: the same steps, spelled out)
                if net64.pool_types[i] is not None:
                    cur = ref_utils.compute_conv_output_sequence_lengths(cur, kernel_size=net64.pool_sizes[i], dilation=1,
                                                                         stride=net64.pool_strides[i], pad_type=net64.pad_types[i])
                seqlens.append(cur)
            out[case + '_seqlens'] = np.array(json.dumps([[int(v) for v in s] for s in seqlens]))
            out[case + '_rf'] = np.asarray(net64.get_receptive_field()).astype(np.int64)
        print(case, 'worst share %.3f (%s)' % (max(sh.values()), max(sh, key=sh.get)))
        worst = max(worst, max(sh.values()))
        if case == 'n0':
            # the evaluation pass after two training passes (the first was the run above), with the buffers they left
            run(case, mods, torch.float64, net64)
            net64.eval()
            with torch.no_grad():
                y = net64(torch.from_numpy(inputs(case)).to(torch.float64), list(LENGTHS))[0]
            out['n0e_y64'] = y.numpy().copy()
            for k, v in net64.state_dict().items():
                if 'running' in k or 'num_tracked' in k:
                    out['n0e_b_' + k] = v.numpy().copy()
            run(case, mods, torch.float32, net32)
            net32.eval()
            with torch.no_grad():
                y32 = net32(torch.from_numpy(inputs(case)), list(LENGTHS))[0].numpy()
            share = float(np.abs(y32 - out['n0e_y64']).max()) / (VALUE * float(np.abs(out['n0e_y64']).max()))
            print('n0 evaluation pass: share %.3f' % share)
            worst = max(worst, share)
    for pad in POOL_PADS:
        res = []
        for dtype in (torch.float64, torch.float32):
            x = torch.from_numpy(pool_inputs(pad)).to(dtype).requires_grad_()
            y, lens, idx = ref_utils.Pool1d('max', 3, 2, pad)(x, np.asarray(POOL_LENGTHS))
            _, r0 = pool_inputs(pad, tuple(y.shape))
            g, = torch.autograd.grad((y * torch.from_numpy(r0).to(dtype)).sum(), [x])
            res.append({'y': y.detach().numpy().copy(), 'g_x': g.numpy().copy(), 'idx': idx.numpy().copy(), 'len': np.asarray(lens)})
        front, end = ref_utils.compute_pad_size(3, 1, 2, pad)
        assert (front, end) == pad_size(3, 2, pad), (pad, front, end)
        assert unique_maximum(pool_inputs(pad), res[0]['idx'].shape[2], 3, 2, front, end).all(), f'Pool1d {pad}: a window holds a tie'
        assert np.array_equal(res[0]['idx'], res[1]['idx'])
        sh = shares(res[1], res[0])
        store(out, f'q_{pad}_', res[0], res[1])
        print('Pool1d', pad, 'shares: ' + ' '.join('%s %.3f' % kv for kv in sh.items()))
        worst = max(worst, max(sh.values()))
    assert worst <= SHARE, f'the reference\'s fp32 run is {worst:.3f} of a gate from its fp64 run (limit {SHARE})'
    out['lengths'] = np.array(LENGTHS)
    path = HERE / 'g26_je_conv.npz'
    np.savez_compressed(path, **out)
    print(path, path.stat().st_size, 'bytes; worst share %.3f' % worst)


if __name__ == '__main__':
    main()
