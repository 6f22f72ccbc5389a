#!/usr/bin/env python3
"""Generate tests/golden/g15_tasnet.npz by importing the REAL reference's TasNet (padertorch/contrib/examples/source_separation/tasnet/
model.py) with its TasEncoder, TasDecoder and ConvNet.

Run in the build container only (needs /root/reference):

    python tests/golden/make_golden_tasnet.py

The reference is imported exactly as make_golden_convnet.py does.  The output is data only.  Four configurations (CASES below):

    0  L 16, N 12 -> separator 8 / 16, 2x1 gLN, K 2, sigmoid, masked, B 3, T 203 (padded: 203 is no multiple of 8), lengths 203 150 97
    1  L 16, N 8, 2x1 cLN, K 3, additional output 5, relu, masked, B 2, T 208 (unpadded: the "minus one" branch), lengths 208 64
    2  L 10, encoder 10 / decoder 6 features, separator 7 / 9, 1x1 gLN, K 2, tanh, mask=False, B 1, T 57
    3  L 2, stride 1 (the win2 configuration), N 5, separator 4 / 8, 2x1 gLN, K 2, additional output 3, identity, masked, B 2, T 64, lengths 64 31

``inputs(case, seed)`` draws the mixtures ``y [B, T]`` (random over the whole padded length: no frame of the encoder is exactly zero), the
targets ``s [B, K, T]`` and the weights ``r [B, K, T]`` / ``r2 [B, A, E]`` of the functional ``sum(out r) + sum(additional_out r2)`` from a
seeded numpy RandomState; they are NOT stored, the tests call the same function.  The norms' gains are drawn from [0.5, 1.5], their offsets
from [-0.5, 0.5], the PReLU slopes from [0.1, 0.4], as in g14.

Ties: per case the seed is moved until no input of a ReLU / PReLU of the fp64 run (the encoder's pre-activation, the separator's PReLUs,
output_prelu, a relu / prelu output nonlinearity) lies within 1e-5 max|input| of zero, and until the reference's own fp32 run agrees with
its fp64 run to half the tests' gates (values 1e-5 max|want|, gradients 2e-4 max|want|) in every stored quantity.  ``c<i>_margin`` and
``c<i>_seed`` are stored.

Keys per case ``c<i>_``: ``keys`` / ``names`` (json lists: state_dict keys, named_parameters), ``p_<key>``, ``lengths`` (encoded_sequence_lengths),
``out64`` / ``out32``, ``add64`` / ``add32`` (A > 0), ``loss64`` / ``loss32`` ([si-sdr, log-mse, log1p-mse]), ``gf64_<name>`` / ``gf32_<name>``
the gradients of the functional and ``gl64_<name>`` / ``gl32_<name>`` those of the si-sdr loss w.r.t. every named parameter and ``y``
(name ``y``).  ``audio_*`` / ``review_keys``: what the reference's ``summary.audio`` and ``summary.review_dict`` return.
"""
import json
import sys
from pathlib import Path

HERE = Path(__file__).resolve().parent
REPO = HERE.parent.parent

import numpy as np  # noqa: E402

CASES = [
    dict(L=16, stride=None, n_enc=12, n_dec=12, sep_in=8, hidden=16, blocks=2, repeats=1, norm='gLN', K=2, A=0, nonlinearity='sigmoid',
         mask=True, B=3, T=203, num_samples=[203, 150, 97]),
    dict(L=16, stride=None, n_enc=8, n_dec=8, sep_in=8, hidden=16, blocks=2, repeats=1, norm='cLN', K=3, A=5, nonlinearity='relu',
         mask=True, B=2, T=208, num_samples=[208, 64]),
    dict(L=10, stride=None, n_enc=10, n_dec=6, sep_in=7, hidden=9, blocks=1, repeats=1, norm='gLN', K=2, A=0, nonlinearity='tanh',
         mask=False, B=1, T=57, num_samples=[57]),
    dict(L=2, stride=1, n_enc=5, n_dec=5, sep_in=4, hidden=8, blocks=2, repeats=1, norm='gLN', K=2, A=3, nonlinearity='identity',
         mask=True, B=2, T=64, num_samples=[64, 31]),
]
TIE_MARGIN = 1e-5
VALUE, GRAD = 1e-5, 2e-4
LOSSES = ['si-sdr', 'log-mse', 'log1p-mse']


def frames(case):
    """Frames the encoder returns for the padded batch (tas_coders.py:73-87)."""
    h = case['L'] // 2
    stride = h if case['stride'] is None else case['stride']
    padded = case['T'] if case['T'] % h == 0 else case['T'] + h - case['T'] % h
    return (padded - case['L']) // stride + 1


def inputs(case, seed):
    """``(y [B, T], s [B, K, T], r [B, K, T], r2 [B, A, E])``, float32."""
    rng = np.random.RandomState(seed)
    B, K, T, A = case['B'], case['K'], case['T'], case['A']
    return (rng.randn(B, T).astype(np.float32), rng.randn(B, K, T).astype(np.float32), rng.randn(B, K, T).astype(np.float32),
            rng.randn(B, A, frames(case)).astype(np.float32))


def parameter_range(name):
    """The range a parameter is redrawn from, or None to keep its initialisation."""
    leaf = name.rsplit('.', 1)[1]
    if 'activation_fn' in name or name.startswith(('output_prelu', 'output_nonlinearity')):
        return 0.1, 0.4
    if '.conv.' not in name and 'norm' in name and leaf in ('gamma', 'weight'):
        return 0.5, 1.5
    if '.conv.' not in name and 'norm' in name and leaf in ('beta', 'bias'):
        return -0.5, 0.5
    return None


def build(case, seed):
    import torch
    from padertorch.contrib.examples.source_separation.tasnet.model import TasNet  # the reference
    from padertorch.contrib.examples.source_separation.tasnet.tas_coders import TasDecoder, TasEncoder
    from padertorch.modules.convnet import ConvNet
    torch.manual_seed(seed)
    net = TasNet(TasEncoder(case['L'], case['n_enc'], case['stride']),
                 ConvNet(input_size=case['sep_in'], num_blocks=case['blocks'], num_repeats=case['repeats'], hidden_channels=case['hidden'],
                         kernel_size=3, norm=case['norm']),
                 TasDecoder(case['L'], case['n_dec'], case['stride']), mask=case['mask'], output_nonlinearity=case['nonlinearity'],
                 num_speakers=case['K'], additional_out_size=case['A'])
    rng = np.random.RandomState(seed + 1)
    with torch.no_grad():
        for name, p in net.named_parameters():
            span = parameter_range(name)
            if span is not None:
                p.copy_(torch.from_numpy(rng.uniform(*span, size=tuple(p.shape)).astype(np.float32)))
    return net


def run(net, case, seed, dtype, margins=None):
    """One forward, the functional's and the si-sdr loss's gradients."""
    import torch
    y0, s0, r0, r20 = inputs(case, seed)
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
    batch = dict(y=list(y.unbind(0)), s=torch.from_numpy(s0).to(dtype), num_samples=list(case['num_samples']))
    out = net(batch)
    for h in hooks:
        h.remove()
    losses = net.loss(batch, out)
    names = [n for n, _ in net.named_parameters()]
    leaves = [p for _, p in net.named_parameters()] + [y]
    functional = (out['out'] * torch.from_numpy(r0).to(dtype)).sum()
    if case['A']:
        functional = functional + (out['additional_out'] * torch.from_numpy(r20).to(dtype)).sum()
    gf = torch.autograd.grad(functional, leaves, retain_graph=True)
    gl = torch.autograd.grad(losses['si-sdr'], leaves)
    res = dict(out=out['out'].detach().numpy().copy(), loss=np.array([float(losses[k].detach()) for k in LOSSES]),
               lengths=np.asarray(out['encoded_sequence_lengths']).astype(np.int64))
    if case['A']:
        res['add'] = out['additional_out'].detach().numpy().copy()
    for n, a, b in zip(names + ['y'], gf, gl):
        res['gf_' + n], res['gl_' + n] = a.numpy().copy(), b.numpy().copy()
    assert tuple(out['encoded'].shape) == (case['B'], frames(case), case['n_enc']), out['encoded'].shape
    return res, names


def ratios(r32, r64):
    """{quantity: |fp32 - fp64| / (gate max|fp64|)} of the reference's two runs."""
    out = {}
    for k, want in r64.items():
        if k == 'lengths':
            continue
        gate = GRAD if k.startswith(('gf_', 'gl_')) else VALUE
        scale = float(np.abs(want).max())
        err = float(np.abs(r32[k].astype(np.float64) - want).max())
        out[k] = err / (gate * scale) if scale > 0 else (0. if err == 0 else float('inf'))
    return out


def main():
    sys.path[:0] = [str(HERE / 'ref_shim'), str(REPO), '/root/reference']
    import torch
    import padertorch as pt

    torch.set_num_threads(1)
    torch.use_deterministic_algorithms(True)
    out = {}
    for i, case in enumerate(CASES):
        seed = 1500 + 100 * i
        while True:
            net = build(case, seed)
            params = {k: v.numpy().copy() for k, v in net.state_dict().items()}
            margins = []
            r64, names = run(net, case, seed, torch.float64, margins)
            if min(margins) >= TIE_MARGIN:
                r32, _ = run(build(case, seed), case, seed, torch.float32)
                rat = ratios(r32, r64)
                if max(rat.values()) <= 0.5:
                    break
                print(case, 'seed', seed, 'fp32 against fp64 above half a gate:', max(rat, key=rat.get), max(rat.values()))
            seed += 1
        p = f'c{i}_'
        out[p + 'seed'], out[p + 'margin'] = np.array(seed), np.array(min(margins))
        out[p + 'keys'] = np.array(json.dumps(list(params)))
        out[p + 'names'] = np.array(json.dumps(names))
        for k, v in params.items():
            out[p + 'p_' + k] = v
        out[p + 'lengths'] = r64['lengths']
        for k in r64:
            if k != 'lengths':
                head, _, tail = k.partition('_')
                name64, name32 = (head + '64', head + '32') if not tail else (head + '64_' + tail, head + '32_' + tail)
                out[p + name64], out[p + name32] = r64[k], r32[k]
        groups = {'out': ['out'], 'additional_out': ['add'], 'losses': ['loss'],
                  'functional gradients': [k for k in rat if k.startswith('gf_')], 'si-sdr gradients': [k for k in rat if k.startswith('gl_')]}
        print(i, 'seed', seed, 'margin %.2e' % min(margins), 'fp32 vs fp64 as a share of the gate:',
              ', '.join('%s %.3f' % (g, max(rat[k] for k in ks if k in rat)) for g, ks in groups.items() if any(k in rat for k in ks)))
    # host helpers of the review
    rng = np.random.RandomState(7)
    sig = rng.randn(2, 50).astype(np.float32)
    out['audio_in'] = sig
    a, rate = pt.summary.audio(signal=torch.from_numpy(sig[0]), sampling_rate=8000)
    out['audio_out'], out['audio_rate'] = np.asarray(a), np.array(rate)
    a, rate = pt.summary.audio(signal=sig, batch_first=True, normalize=False)
    out['audio_out_batch_first'], out['audio_rate_default'] = np.asarray(a), np.array(rate)
    a, _ = pt.summary.audio(signal=sig.T)
    out['audio_out_batch_second'] = np.asarray(a)
    a, _ = pt.summary.audio(signal=np.zeros(4, np.float32))
    out['audio_out_zeros'] = np.asarray(a)
    review = pt.summary.review_dict(losses={'a': torch.tensor(1.)}, audios={'b': (sig[0], 8000)})
    out['review_keys'] = np.array(json.dumps(list(review)))
    out['cases'] = np.array(json.dumps(CASES))
    path = HERE / 'g15_tasnet.npz'
    np.savez_compressed(path, **out)
    print(path, path.stat().st_size, 'bytes')


if __name__ == '__main__':
    main()
