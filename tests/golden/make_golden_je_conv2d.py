#!/usr/bin/env python3
"""Generate tests/golden/g27_je_conv2d.npz by importing the REAL reference's 2-D convolution stack and hybrids
(padertorch/contrib/je/modules/conv.py, conv_utils.py, hybrid.py).

Run in the build container only (needs /root/reference and einops):

    python tests/golden/make_golden_je_conv2d.py

The pattern is make_golden_je_conv.py's; ``shares`` and ``store`` are that module's.  The output is data only: parameters and the results
of an fp64 and an fp32 run of the reference.  Inputs are NOT stored: ``inputs`` draws them from a seeded numpy RandomState and the tests
call the same function.  All cases run on ``x [3, 1, 12, 21]`` with lengths ``[21, 17, 9]`` (random values behind the lengths too),
functional ``sum(y * r)``; biases, ``gamma`` and ``beta`` carry a seeded perturbation of 0.3 N(0, 1).  ``CASES`` lists the constructors
(a dict: the keyword arguments of a hybrid, nested entries built by ``assemble``).  Keys per case as in g26; for the ``CNN2d`` cases also ``shapes``, ``seqlens``, ``rf``;
``w0e_``: an evaluation pass of ``w0`` after two training passes; ``p2_<i>_len``: ``Pool2d`` output lengths of ``POOLS[i]``.

The reference's own fp32 run must stay within a QUARTER of every gate; the generator prints the shares and refuses to write otherwise.
"""
import importlib.util
import json
import sys
from pathlib import Path

HERE = Path(__file__).resolve().parent
REPO = HERE.parent.parent

import numpy as np  # noqa: E402

_spec = importlib.util.spec_from_file_location('make_golden_je_conv', HERE / 'make_golden_je_conv.py')
g26 = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(g26)

SHAPE, LENGTHS, CONDITION = (3, 1, 12, 21), [21, 17, 9], (3, 2)
SHARE = 0.25
#: Pool2d(pool_type, size, stride, pad_type) whose output lengths are stored
POOLS = [('max', (2, 2), None, None), ('max', (2, 2), None, 'both'), ('avg', (3, 2), (1, 2), ('front', None)), ('max', (1, 3), None, 'end')]

#: name -> (class name, positional arguments, keyword arguments) or (class name, keyword arguments with nested entries)
CASES = {
    'w0': ('CNN2d', (1, [6, 10, 5], [3, 3, 2]), dict(pad_type=['both', 'both', None], pool_size=[1, 2, 1], norm='batch')),
    'w1': ('CNN2d', (1, [6, 6, 8, 5], 3), dict(residual_connections=[None, 3, None, None], dense_connections=[None, 2, None, None],
                                               pre_activation=True, gated=True, norm='batch')),
    'w2': ('CNN2d', (1, [4, 6], 3), dict(norm='sequence', pool_size=[2, 1], return_pool_indices=True, activation_fn='elu')),
    'h0': ('CNN', dict(cnn_2d=dict(in_channels=4, out_channels=[4, 4], kernel_size=3, pool_size=[2, 1], norm='batch'),
                       cnn_1d=dict(in_channels=4 * 6 + 2, out_channels=[8, 5], kernel_size=3),
                       input_height=12, conditional_dims=2, positional_encoding=True)),
    'h1': ('CRNN', dict(cnn_2d=dict(in_channels=1, out_channels=[8, 8, 4], kernel_size=3),
                        cnn_1d=dict(in_channels=4 * 12, out_channels=[8, 8, 4], kernel_size=3),
                        rnn=dict(input_size=4, hidden_size=6, num_layers=1, bias=True, batch_first=True, dropout=0., bidirectional=False),
                        fcn=dict(input_size=6, hidden_size=8, output_size=5, dropout=0.), input_size=12)),
}
#: the factories of the nested entries of a hybrid's keyword arguments (the reference's own config system needs a package that is not
#: installed here, so the hybrids are assembled from resolved configs; ``finalize_dogmatic_config`` has a host test of its own)
PARTS = {'cnn_2d': 'CNN2d', 'cnn_1d': 'CNN1d', 'rnn': 'GRU', 'fcn': 'fully_connected_stack'}


def assemble(cls, kwargs, mods):
    """``mods[cls]`` with its nested entries built by ``mods[PARTS[key]]``."""
    return mods[cls](**{k: mods[PARTS[k]](**v) if k in PARTS else v for k, v in kwargs.items()})


def seed_of(case):
    return 2700 + sorted(CASES).index(case)


def inputs(case, out_shape=None):
    """``x`` float32, the condition (``h0`` only, else None) and, with ``out_shape``, ``r``."""
    rng = np.random.RandomState(seed_of(case))
    x = rng.randn(*SHAPE).astype(np.float32)
    cond = rng.randn(*CONDITION).astype(np.float32) if case == 'h0' else None
    return (x, cond) if out_shape is None else (x, cond, rng.randn(*out_shape).astype(np.float32))


def build(case, mods, dtype):
    """The module of ``case`` from the classes ``mods`` with seeded, perturbed parameters."""
    import torch
    cls, *spec = CASES[case]
    torch.manual_seed(seed_of(case))
    net = mods[cls](*spec[0], **spec[1]) if len(spec) == 2 else assemble(cls, spec[0], mods)
    rng = np.random.RandomState(100 + seed_of(case))
    with torch.no_grad():
        for name, p in net.named_parameters():
            if name.endswith(('bias', 'gamma', 'beta')) or '.bias_' in name:
                p.add_(torch.from_numpy(0.3 * rng.randn(*p.shape)).to(p.dtype))
    return net.to(dtype)


def call(case, net, x, cond):
    return net(x, list(LENGTHS), cond) if case == 'h0' else net(x, list(LENGTHS))


def run(case, mods, dtype, net=None):
    import torch
    net = build(case, mods, dtype) if net is None else net
    x0, c0 = inputs(case)
    x = torch.from_numpy(x0).to(dtype).requires_grad_()
    out = call(case, net, x, None if c0 is None else torch.from_numpy(c0).to(dtype))
    y = out[0]
    r0 = inputs(case, tuple(y.shape))[2]
    named = list(net.named_parameters())
    grads = torch.autograd.grad((y * torch.from_numpy(r0).to(dtype)).sum(), [x] + [p for _, p in named])
    res = {'y': y.detach().numpy().copy(), 'g_x': grads[0].numpy().copy(), 'len': np.asarray(out[1])}
    for (n, _), g in zip(named, grads[1:]):
        res['g_' + n] = g.numpy().copy()
    if case == 'w2':
        for i, idx in enumerate(out[2]):
            if idx is not None:
                res[f'idx{i}'] = idx.numpy().copy()
    return res, net


def main():
    sys.path[:0] = [str(HERE / 'ref_shim'), str(REPO), '/root/reference']
    if not hasattr(np, 'int'):
        np.int = int                    # the reference's get_receptive_field still says np.int
    import torch
    from padertorch.contrib.je.modules import conv as ref_conv  # the reference
    from padertorch.contrib.je.modules import conv_utils as ref_utils
    from padertorch.contrib.je.modules import hybrid as ref_hybrid

    torch.set_num_threads(1)
    torch.use_deterministic_algorithms(True)
    from padertorch.modules.fully_connected import fully_connected_stack
    mods = {'CNN2d': ref_conv.CNN2d, 'CNN1d': ref_conv.CNN1d, 'CNN': ref_hybrid.CNN, 'CRNN': ref_hybrid.CRNN, 'GRU': torch.nn.GRU,
            'fully_connected_stack': fully_connected_stack}
    out, worst = {}, 0.
    for case in CASES:
        r64, net64 = run(case, mods, torch.float64)
        r32, net32 = run(case, mods, torch.float32)
        sh = g26.shares(r32, r64)
        state = build(case, mods, torch.float32).state_dict()
        out[case + '_keys'] = np.array(json.dumps(list(state)))
        out[case + '_names'] = np.array(json.dumps([n for n, _ in net32.named_parameters()]))
        for k, v in state.items():
            out[f'{case}_p_{k}'] = v.numpy().copy()
        g26.store(out, case + '_', r64, r32)
        if case.startswith('w'):
            out[case + '_shapes'] = np.array(json.dumps([[int(v) for v in s] for s in net64.get_shapes(input_shape=SHAPE)]))
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
        if case == 'w0':
            # the evaluation pass after two training passes (the first was the run above), with the buffers they left
            run(case, mods, torch.float64, net64)
            net64.eval()
            with torch.no_grad():
                y = net64(torch.from_numpy(inputs(case)[0]).to(torch.float64), list(LENGTHS))[0]
            out['w0e_y64'] = y.numpy().copy()
            for k, v in net64.state_dict().items():
                if 'running' in k or 'num_tracked' in k:
                    out['w0e_b_' + k] = v.numpy().copy()
    for i, (kind, size, stride, pad) in enumerate(POOLS):
        x = torch.zeros(SHAPE, dtype=torch.float64)
        y, lens, _ = ref_utils.Pool2d(kind, size, stride, pad)(x, np.asarray(LENGTHS))
        out[f'p2_{i}_len'], out[f'p2_{i}_shape'] = np.asarray(lens), np.asarray(y.shape)
    assert worst <= SHARE, f'the reference\'s fp32 run is {worst:.3f} of a gate from its fp64 run (limit {SHARE})'
    path = HERE / 'g27_je_conv2d.npz'
    np.savez_compressed(path, **out)
    print(path, path.stat().st_size, 'bytes; worst share %.3f' % worst)


if __name__ == '__main__':
    main()
