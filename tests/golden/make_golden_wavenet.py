#!/usr/bin/env python3
"""Generate tests/golden/g22_wavenet.npz by running the REAL reference's WaveNet (padertorch/modules/wavenet/wavenet.py) and mu-law
companding (padertorch/ops/mu_law.py) on the CPU in fp64 and fp32.

Run in the build container only (needs /root/reference):

    python tests/golden/make_golden_wavenet.py

The reference is imported exactly as make_golden_convnet.py does.  The output is data only.

The reference's ``forward`` applies ``cond_layers`` a second time to what ``get_cond_input`` returns, which raises for every real
configuration.  The maker runs the reference's own ``forward`` text and lets the SECOND call pass its input through (``EveryOtherCall``
below, a module of ours in the place of ``cond_layers``): one application, the network ``infer`` and ``export_weights`` describe.

Configuration: 5 conditioning channels, window 10, stride 4, fading 'full', 256 input classes (the reference's ``forward`` encodes with
mu = 256 whatever ``n_in_channels`` says), L = 7 layers with max_dilation 4 (dilations 1, 2, 4, 1, 2, 4, 1), R = 24, S = 40, A = 16,
B = 2, 12 frames -> 42 conditioning columns, T = 41 samples.

Keys: ``config`` / ``keys`` / ``names`` (json), ``p_<key>`` every state_dict entry, ``features``, ``audio``, ``w`` (the weights of the
functional ``sum(output * w)``), ``output64``, ``quantized``, ``g64_<name>`` for every parameter and for ``features`` (the fp32 run is kept only as its deviations),
 ``dev32_<quantity>`` = max|q32 - q64| / max|q64|, ``cond_full`` / ``cond_half`` / ``cond_none`` (``get_cond_input`` in fp64 for the
three fadings, of the first example alone: they are most of the file), ``mu_x`` / ``mu_codes`` (mu = 256) / ``mu_codes16`` (mu = 16), ``mu_decode`` (all 256 codes) / ``mu_decode16`` (fp32: the reference's
decode converts its input with ``.float()``).

Asserted here (the seed moves if one fails): every ``dev32_*`` is below a quarter of its gate (1e-5 for values, 2e-4 for gradients, of
max|want|); no mu-law input has its pre-rounding value ``(x_mu + 1) / 2 * mu + 0.5`` (fp64) within 1e-3 of an integer, so codes must match
exactly (x = 0, whose value is an integer in every precision, is appended behind that check).
"""
import json
import sys
from pathlib import Path

HERE = Path(__file__).resolve().parent
REPO = HERE.parent.parent

import numpy as np  # noqa: E402

CONFIG = dict(C=5, window=10, stride=4, fading='full', A_in=256, L=7, max_dilation=4, R=24, S=40, A=16, B=2, Tf=12, T=41)
VALUE, GRAD, TIE = 1e-5, 2e-4, 1e-3


def pre_rounding(x, q):
    mu = q - 1.0
    return (np.sign(x) * np.log1p(mu * np.abs(x)) / np.log1p(mu) + 1) / 2 * mu + 0.5


def no_ties(x, q):
    v = pre_rounding(x.astype(np.float64), q)
    return float(np.abs(v - np.round(v)).min()) > TIE


def draw_without_ties(rng, shape, qs):
    while True:
        x = rng.uniform(-1, 1, size=shape).astype(np.float32)
        if all(no_ties(x, q) for q in qs):
            return x


def main():
    sys.path[:0] = [str(HERE / 'ref_shim'), str(REPO), '/root/reference']
    import torch
    from padertorch.modules.wavenet import WaveNet          # the reference
    from padertorch.ops import mu_law_decode, mu_law_encode

    class EveryOtherCall(torch.nn.Module):
        """``inner`` on the 1st, 3rd, ... call, the identity on the 2nd, 4th, ..."""

        def __init__(self, inner):
            super().__init__()
            self.inner, self.calls = inner, 0

        def forward(self, x):
            self.calls += 1
            return self.inner(x) if self.calls % 2 else x

    torch.set_num_threads(1)
    torch.use_deterministic_algorithms(True)
    c = CONFIG
    seed = 2200
    while True:
        torch.manual_seed(seed)
        rng = np.random.RandomState(seed)
        net = WaveNet(c['C'], c['window'], c['stride'], n_in_channels=c['A_in'], n_layers=c['L'], max_dilation=c['max_dilation'],
                      n_residual_channels=c['R'], n_skip_channels=c['S'], n_out_channels=c['A'], fading=c['fading'])
        keys = list(net.state_dict())
        named = dict(net.named_parameters())
        params = {k: v.numpy().copy() for k, v in net.state_dict().items()}
        net.cond_layers = EveryOtherCall(net.cond_layers)
        features = rng.randn(c['B'], c['C'], c['Tf']).astype(np.float32)
        audio = draw_without_ties(rng, (c['B'], c['T']), (256,))
        w = rng.randn(c['B'], c['A'], c['T']).astype(np.float32)

        def run(dtype):
            net.to(dtype)
            for p in net.parameters():
                p.grad = None
            net.cond_layers.calls = 0
            f = torch.from_numpy(features).to(dtype).requires_grad_()
            out, quantized = net(f, torch.from_numpy(audio).to(dtype))
            (out * torch.from_numpy(w).to(dtype)).sum().backward()
            grads = {k: p.grad.numpy().copy() for k, p in named.items()}
            grads['features'] = f.grad.numpy().copy()
            return out.detach().numpy().copy(), quantized.numpy().copy(), grads

        out64, q64, g64 = run(torch.float64)
        conds = {}
        for fading in ('full', 'half', None):
            net.fading, net.cond_layers.calls = fading, 0
            with torch.no_grad():
                conds[str(fading).lower()] = net.get_cond_input(torch.from_numpy(features[:1]).double()).numpy().copy()
        net.fading = c['fading']
        out32, q32, g32 = run(torch.float32)

        def dev(a, b):
            return float(np.abs(a.astype(np.float64) - b).max() / np.abs(b).max())
        devs = {'output': dev(out32, out64), **{k: dev(g32[k], g64[k]) for k in g64}}
        ok = devs['output'] < VALUE / 4 and all(v < GRAD / 4 for k, v in devs.items() if k != 'output') and (q32 == q64).all()
        print('seed', seed, 'fp32 vs fp64: output %.1e, worst gradient %.1e (%s)' % (
            devs['output'], max(v for k, v in devs.items() if k != 'output'), max((k for k in devs if k != 'output'), key=devs.get)))
        if ok:
            break
        seed += 1

    # (x = 0 is appended behind the check: its pre-rounding value (mu + 1) / 2 IS an integer, but exactly so in every precision)
    mu_x = np.concatenate([draw_without_ties(rng, (300,), (256, 16)), np.array([-1., 1.], dtype=np.float32)])
    assert no_ties(mu_x, 256) and no_ties(mu_x, 16)
    mu_x = np.concatenate([mu_x, np.zeros(1, dtype=np.float32)])
    codes = mu_law_encode(torch.from_numpy(mu_x).double()).numpy()
    codes16 = mu_law_encode(torch.from_numpy(mu_x).double(), 16).numpy()
    assert (mu_law_encode(torch.from_numpy(mu_x)).numpy() == codes).all()
    out = dict(config=np.array(json.dumps(c)), keys=np.array(json.dumps(keys)), names=np.array(json.dumps(list(g64))), seed=np.array(seed),
               features=features, audio=audio, w=w, output64=out64, quantized=q64,
               cond_full=conds['full'], cond_half=conds['half'], cond_none=conds['none'],
               mu_x=mu_x, mu_codes=codes, mu_codes16=codes16,
               mu_decode=mu_law_decode(torch.arange(256).double()).numpy(), mu_decode16=mu_law_decode(torch.arange(16).double(), 16).numpy())
    for k, v in params.items():
        out['p_' + k] = v
    for k in g64:
        out['g64_' + k], out['dev32_' + k] = g64[k], np.array(devs[k])
    out['dev32_output'] = np.array(devs['output'])
    path = HERE / 'g22_wavenet.npz'
    np.savez_compressed(path, **out)
    print(path, path.stat().st_size, 'bytes')


if __name__ == '__main__':
    main()
