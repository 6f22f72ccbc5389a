#!/usr/bin/env python3
"""Generate tests/golden/g18_stft_tasnet.npz by importing the REAL reference's StftEncoder / IstftDecoder (padertorch/contrib/examples/
source_separation/tasnet/tas_coders.py:138-240) and its TasNet around them, with a ConvNet and with a DPRNN separator: the ``stft``
configuration of the reference's TasNet example (tasnet/train.py:119-134).

Run in the build container only (needs /root/reference):

    python tests/golden/make_golden_stft_tasnet.py

The reference is imported exactly as make_golden_tasnet.py does, whose ``parameter_range`` / ``ratios`` this generator uses; the DPRNN
case patches ``paderbox.array.segment_axis`` and checks the reference's doctests through it, as make_golden_dprnn.py does (its
``segment_axis`` / ``check_doctests`` / ``redraw``).  The output is data only.

Model cases (CASES):

    0  L 16, N 64 (size 62, no power of two), hop 8 -> ConvNet 8 / 16, 2x1 gLN, K 2, sigmoid, masked, B 3, T 203 (25 frames, the last
       one padded), lengths 203 150 97
    1  L 16, N 34, stride 4 (four frames cover a sample), 2x1 cLN, K 3, additional output 5, relu, masked, B 2, T 208 (exactly 49 frames,
       nothing padded), lengths 208 64
    2  L 20, N 22 (size == window), 1x1 gLN, K 2, tanh, mask=False, B 1, T 57
    3  the coders of case 0 around DPRNN(8, 8, 6, 3, 1), K 2, sigmoid, masked, B 2, T 203, lengths 203 120 (descending, and the first
       example reaches every chunk: the reference needs both, see make_golden_dprnn.py)

``inputs(case, seed)`` draws the mixtures ``y [B, T]`` (random over the whole padded length), the targets ``s [B, K, T]`` and the weights
``r [B, K, T]`` / ``r2 [B, A, E]`` of the functional ``sum(out r) + sum(additional_out r2)`` from a seeded numpy RandomState; they are NOT
stored, the tests call the same function.  Parameters are redrawn as in g15 / g17.

Ties: per case the seed is moved until no input of a ReLU / PReLU of the fp64 run lies within 1e-5 max|input| of zero (the STFT encoder
itself has no nonlinearity; of the input of ``output_prelu`` the frames of the encoded signal count: a DPRNN returns a few more, exactly
zero for the shorter examples, and TasNet drops them), and until the reference's own fp32 run agrees with its fp64 run to half the tests'
gates (values 1e-5 max|want|, gradients 2e-4 max|want|) in every stored quantity.  ``c<i>_margin`` and ``c<i>_seed`` are stored.

Keys per model case ``c<i>_``: as in g15 (``keys``, ``names``, ``p_<key>``, ``lengths``, ``out64`` / ``out32``, ``add64`` / ``add32``,
``loss64`` / ``loss32``, ``gf64_<name>`` / ``gf32_<name>``, ``gl64_<name>`` / ``gl32_<name>``, name ``y`` for the mixtures).

Coder geometries (GEOMETRIES: (L, N, stride, B, T, K)), keys ``k<j>_``: the reference's ``stft_kernel [N, 1, L]`` and ``istft_kernel_real`` /
``istft_kernel_imag [size, 1, L]`` in fp64; for ``coder_inputs(geometry, seed)`` (``x [B, T]``, ``w [B, N, E]``, ``mask [K, B, N, E]`` and the
weights ``rx [B, N, E]``, ``ry [B, T']``, ``rm [K, B, T']``; the seed is ``k<j>_seed``) the fp64 results ``enc`` = encoder(x), ``dec`` = decoder(w),
``mdec[k]`` = decoder(mask[k] * w) and the gradients ``g_x`` of sum(enc rx), ``g_w`` of sum(dec ry), ``g_mask`` / ``g_enc`` of sum(mdec rm);
``frames_n`` / ``frames`` = ``samples_to_frames(n)`` for n in 1, 5, L-1, L, L+1, L+stride, L+stride+1, 97, 150, 203 (zero or negative
below one window, as the reference returns it).

Frame-count edges, keys ``e<T>_`` for T in 16, 15, 17 with the coders of case 0: ``x [1, T]`` (stored), ``enc`` and ``dec`` = decoder(enc), fp64.
"""
import json
import sys
from pathlib import Path

HERE = Path(__file__).resolve().parent
REPO = HERE.parent.parent

import numpy as np  # noqa: E402

CONVNET = dict(kind='convnet', sep_in=8, hidden=16, repeats=1)
CASES = [
    dict(CONVNET, L=16, N=64, stride=None, blocks=2, norm='gLN', K=2, A=0, nonlinearity='sigmoid', mask=True, B=3, T=203,
         num_samples=[203, 150, 97]),
    dict(CONVNET, L=16, N=34, stride=4, blocks=2, norm='cLN', K=3, A=5, nonlinearity='relu', mask=True, B=2, T=208,
         num_samples=[208, 64]),
    dict(CONVNET, L=20, N=22, stride=None, blocks=1, norm='gLN', K=2, A=0, nonlinearity='tanh', mask=False, B=1, T=57, num_samples=[57]),
    dict(kind='dprnn', sep_in=8, rnn_size=8, window=6, hop=3, blocks=1, L=16, N=64, stride=None, K=2, A=0, nonlinearity='sigmoid',
         mask=True, B=2, T=203, num_samples=[203, 120]),
]
#: (L, N, stride, B, T, K)
GEOMETRIES = [(16, 64, None, 2, 203, 2), (16, 34, 4, 2, 75, 3), (20, 22, None, 2, 57, 2)]
EDGES = [16, 15, 17]
TIE_MARGIN = 1e-5
VALUE, GRAD = 1e-5, 2e-4
LOSSES = ['si-sdr', 'log-mse', 'log1p-mse']


def hop(L, stride):
    return L // 2 if stride is None else stride


def frames_of(samples, L, stride):
    """``ceil((samples - L) / stride) + 1`` frames, one for anything shorter than a window."""
    return max(-((L - samples) // hop(L, stride)) + 1, 1)


def frames(case):
    return frames_of(case['T'], case['L'], case['stride'])


def inputs(case, seed):
    """``(y [B, T], s [B, K, T], r [B, K, T], r2 [B, A, E])``, float32."""
    rng = np.random.RandomState(seed)
    B, K, T, A = case['B'], case['K'], case['T'], case['A']
    return (rng.randn(B, T).astype(np.float32), rng.randn(B, K, T).astype(np.float32), rng.randn(B, K, T).astype(np.float32),
            rng.randn(B, A, frames(case)).astype(np.float32))


def coder_inputs(geometry, seed):
    """``(x [B, T], w [B, N, E], mask [K, B, N, E], rx [B, N, E], ry [B, T'], rm [K, B, T'])``, float32."""
    L, N, stride, B, T, K = geometry
    E = frames_of(T, L, stride)
    Tp = (E - 1) * hop(L, stride) + L
    rng = np.random.RandomState(seed)
    return tuple(rng.randn(*shape).astype(np.float32) for shape in ((B, T), (B, N, E), (K, B, N, E), (B, N, E), (B, Tp), (K, B, Tp)))


def build(case, seed):
    import torch
    from make_golden_dprnn import redraw
    from make_golden_tasnet import parameter_range
    from padertorch.contrib.examples.source_separation.tasnet.model import TasNet  # the reference
    from padertorch.contrib.examples.source_separation.tasnet.tas_coders import IstftDecoder, StftEncoder
    from padertorch.modules.convnet import ConvNet
    from padertorch.modules.dual_path_rnn import DPRNN
    torch.manual_seed(seed)
    if case['kind'] == 'dprnn':
        separator = DPRNN(case['sep_in'], case['rnn_size'], case['window'], case['hop'], case['blocks'])
    else:
        separator = ConvNet(input_size=case['sep_in'], num_blocks=case['blocks'], num_repeats=case['repeats'],
                            hidden_channels=case['hidden'], kernel_size=3, norm=case['norm'])
    net = TasNet(StftEncoder(case['L'], case['N'], case['stride']), separator, IstftDecoder(case['L'], case['N'], case['stride']),
                 mask=case['mask'], output_nonlinearity=case['nonlinearity'], num_speakers=case['K'], additional_out_size=case['A'])
    if case['kind'] == 'dprnn':
        return redraw(net, seed)
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
            t = t.detach()[..., :frames(case)]      # [B, C, frames]: a DPRNN returns frames behind the encoded signal, which TasNet drops
            margins.append(float(t.abs().min() / t.abs().max()))
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
    assert tuple(out['encoded'].shape) == (case['B'], frames(case), case['N']), out['encoded'].shape
    return res, names


def coders(out):
    """The bases, the three operators and the frame arithmetic of the reference's coders, fp64."""
    import torch
    from padertorch.contrib.examples.source_separation.tasnet.tas_coders import IstftDecoder, StftEncoder
    for j, geometry in enumerate(GEOMETRIES):
        L, N, stride, B, T, K = geometry
        seed, p = 1900 + j, f'k{j}_'
        enc, dec = StftEncoder(L, N, stride), IstftDecoder(L, N, stride)
        out[p + 'seed'] = np.array(seed)
        out[p + 'stft_kernel'] = np.asarray(enc.stft.stft_kernel, dtype=np.float64)
        out[p + 'istft_kernel_real'] = np.asarray(dec.stft.istft_kernel_real, dtype=np.float64)
        out[p + 'istft_kernel_imag'] = np.asarray(dec.stft.istft_kernel_imag, dtype=np.float64)
        assert out[p + 'stft_kernel'].shape == (N, 1, L) and out[p + 'istft_kernel_real'].shape == (N - 2, 1, L)
        x, w, mask, rx, ry, rm = (torch.from_numpy(a).double() for a in coder_inputs(geometry, seed))
        x, w, mask = x.requires_grad_(), w.requires_grad_(), mask.requires_grad_()
        e = enc(x)
        y = dec(w)
        my = torch.stack([dec(mask[k] * w) for k in range(K)])
        assert e.shape == rx.shape and y.shape == ry.shape and my.shape == rm.shape, (e.shape, y.shape, my.shape)
        out[p + 'enc'], out[p + 'dec'], out[p + 'mdec'] = e.detach().numpy().copy(), y.detach().numpy().copy(), my.detach().numpy().copy()
        out[p + 'g_x'] = torch.autograd.grad((e * rx).sum(), x)[0].numpy().copy()
        out[p + 'g_w'] = torch.autograd.grad((y * ry).sum(), w)[0].numpy().copy()
        gm, ge = torch.autograd.grad((my * rm).sum(), [mask, w])
        out[p + 'g_mask'], out[p + 'g_enc'] = gm.numpy().copy(), ge.numpy().copy()
        s = hop(L, stride)
        ns = [1, 5, L - 1, L, L + 1, L + s, L + s + 1, 97, 150, 203]
        out[p + 'frames_n'] = np.array(ns, dtype=np.int64)
        out[p + 'frames'] = np.array([int(enc.stft.samples_to_frames(n)) for n in ns], dtype=np.int64)
        print('coders', geometry, 'frames', dict(zip(ns, out[p + 'frames'].tolist())))
    L, N, stride = GEOMETRIES[0][:3]
    enc, dec = StftEncoder(L, N, stride), IstftDecoder(L, N, stride)
    rng = np.random.RandomState(1950)
    for T in EDGES:
        x = rng.randn(1, T)
        e = enc(torch.from_numpy(x))
        out[f'e{T}_x'], out[f'e{T}_enc'], out[f'e{T}_dec'] = x, e.numpy().copy(), dec(e).numpy().copy()
        print('edge', T, 'samples ->', tuple(e.shape), '->', tuple(out[f'e{T}_dec'].shape))


def main():
    sys.path[:0] = [str(HERE), str(HERE / 'ref_shim'), str(REPO), '/root/reference']
    import torch
    import paderbox
    from make_golden_dprnn import check_doctests, segment_axis
    from make_golden_tasnet import ratios

    paderbox.array.segment_axis = segment_axis
    torch.set_num_threads(1)
    torch.use_deterministic_algorithms(True)
    check_doctests()
    out = {}
    for i, case in enumerate(CASES):
        seed = 1800 + 100 * i
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
            else:
                print(case, 'seed', seed, 'tie margin', min(margins))
            seed += 1
        p = f'c{i}_'
        assert not any(k.startswith(('encoder.', 'decoder.')) for k in params), list(params)      # the coders hold no state
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
        print(i, 'seed', seed, 'lengths', r64['lengths'].tolist(), 'margin %.2e' % min(margins), 'fp32 vs fp64 as a share of the gate:',
              ', '.join('%s %.3f' % (g, max(rat[k] for k in ks if k in rat)) for g, ks in groups.items() if any(k in rat for k in ks)))
    coders(out)
    out['cases'] = np.array(json.dumps(CASES))
    out['geometries'] = np.array(json.dumps(GEOMETRIES))
    out['edges'] = np.array(json.dumps(EDGES))
    path = HERE / 'g18_stft_tasnet.npz'
    np.savez_compressed(path, **out)
    print(path, path.stat().st_size, 'bytes')


if __name__ == '__main__':
    main()
