#!/usr/bin/env python3
"""Generate tests/golden/g24_transformer*.npz by running the REAL reference's transformer (padertorch/contrib/je/modules/transformer.py)
on the CPU in fp64 and fp32.

Run in the build container only (needs the reference checkout and einops):

    python tests/golden/make_golden_transformer.py

The reference is imported exactly as make_golden_wavenet.py does.  The output is data only.

Configuration: ``TransformerLayerStack(10, 48, 40, 3, 2)`` (d_model 48, d_ff 40, 3 heads of 16, 2 layers), B = 3, T = 37, seq_len
[37, 20, 1]; biases and beta drawn N(0, 0.3), gamma 1 + 0.3 N(0, 1); the functional is ``sum(y * w)``.  Variants:

    bi_nf, bi_nl      bidirectional, norm_first True / False
    nonorm            norm=None
    batch, batch_b    norm='batch' (training mode: batch statistics), two seeds
    cross             cross_attention=True, m [3, 11, 48], seq_len_m [11, 4, 7]
    causal_state      causal, a 4-frame state per layer
    causal_long       causal, B = 1, T = 200, no lengths

Files: every quantity of a variant is fp64 (27.6 k parameter gradients alone are 221 kB), so one file cannot hold all variants within
the repository's 1 MiB limit per file.  ``g24_transformer.npz`` is the index: ``variants`` (json: per variant its configuration, the
state_dict ``keys``, the gradient ``names`` and ``dev32`` = max|q32 - q64| / max|q64| of every quantity), ``seed``, the ``get_causal_mask``
cases ``causal_5_9`` / ``causal_9_5`` / ``causal_4_4`` and the free function's cases ``sdpa_*`` (q [2, 2, 5, 4], k [2, 2, 9, 4],
v [2, 2, 9, 6], mask [2, 1, 5, 9]; ``out`` and ``weights`` for causal, bidirectional with seq_len [9, 3] and either with the mask).
``g24_transformer_<variant>.npz`` holds ``<variant>/p_<key>`` every state_dict entry (before the run), ``<variant>/x``, ``/w``, ``/m``,
``/state<i>``, ``/y64``, ``/out_state<i>`` and ``/g64_<name>`` for ``x``, ``m`` and every parameter.

Asserted here (the seed moves if it fails): for every variant but the two batch ones, every dev32 is below a quarter of its gate
(1e-5 for values, 2e-4 for gradients; quantities whose fp64 gradient is analytically zero - max|g64| < 1e-12 - are left out).
"""
import json
import sys
from pathlib import Path

HERE = Path(__file__).resolve().parent
REPO = HERE.parent.parent

import numpy as np  # noqa: E402

VALUE, GRAD = 1e-5, 2e-4
BASE = dict(input_size=10, hidden_size=48, d_ff=40, num_heads=3, num_layers=2)
B, T = 3, 37
VARIANTS = {
    'bi_nf': dict(bidirectional=True, cross_attention=False, norm='layer', norm_first=True),
    'bi_nl': dict(bidirectional=True, cross_attention=False, norm='layer', norm_first=False),
    'nonorm': dict(bidirectional=True, cross_attention=False, norm=None, norm_first=True),
    'batch': dict(bidirectional=True, cross_attention=False, norm='batch', norm_first=True),
    'batch_b': dict(bidirectional=True, cross_attention=False, norm='batch', norm_first=True, seed_offset=1000),
    'cross': dict(bidirectional=True, cross_attention=True, norm='layer', norm_first=True),
    'causal_state': dict(bidirectional=False, cross_attention=False, norm='layer', norm_first=True, state=True),
    'causal_long': dict(bidirectional=False, cross_attention=False, norm='layer', norm_first=True, B=1, T=200, seq_len=None),
}


def main():
    sys.path[:0] = [str(HERE / 'ref_shim'), str(REPO), '/root/reference']
    import torch
    from padertorch.contrib.je.modules.transformer import (TransformerLayerStack, get_causal_mask,          # the reference
                                                           scaled_dot_product_attention)

    torch.set_num_threads(1)
    torch.use_deterministic_algorithms(True)

    def dev(a, b):
        return float(np.abs(a.astype(np.float64) - b).max() / max(np.abs(b).max(), 1e-300))

    def run_variant(name, cfg, seed):
        seed = seed + cfg.get('seed_offset', 0)
        torch.manual_seed(seed)
        rng = np.random.RandomState(seed)
        kw = {k: cfg[k] for k in ('bidirectional', 'cross_attention', 'norm', 'norm_first')}
        net = TransformerLayerStack(**BASE, **kw)
        with torch.no_grad():
            for k, p in net.named_parameters():
                if k.endswith('.bias') or k.endswith('.beta'):
                    p.copy_(torch.from_numpy(rng.normal(0, 0.3, size=tuple(p.shape)).astype(np.float32)))
                elif k.endswith('.gamma'):
                    p.copy_(torch.from_numpy((1 + 0.3 * rng.normal(size=tuple(p.shape))).astype(np.float32)))
        keys = list(net.state_dict())
        params = {k: v.numpy().copy() for k, v in net.state_dict().items()}
        named = dict(net.named_parameters())
        b, t = cfg.get('B', B), cfg.get('T', T)
        seq_len = cfg.get('seq_len', [37, 20, 1])
        seq_len_m = [11, 4, 7] if cfg['cross_attention'] else None
        x = rng.randn(b, t, BASE['input_size']).astype(np.float32)
        w = rng.randn(b, t, BASE['hidden_size']).astype(np.float32)
        m = rng.randn(b, 11, BASE['hidden_size']).astype(np.float32) if cfg['cross_attention'] else None
        state = [rng.randn(b, 4, BASE['hidden_size']).astype(np.float32) for _ in range(BASE['num_layers'])] if cfg.get('state') else None

        def run(dtype):
            net.load_state_dict({k: torch.from_numpy(v) for k, v in params.items()})       # (the batch norm's buffers move in a run)
            net.to(dtype)
            net.train()
            for p in net.parameters():
                p.grad = None
            xt = torch.from_numpy(x).to(dtype).requires_grad_()
            mt = None if m is None else torch.from_numpy(m).to(dtype).requires_grad_()
            st = None if state is None else [torch.from_numpy(s).to(dtype) for s in state]
            y, states = net(xt, seq_len, m=mt, seq_len_m=seq_len_m, state=st)
            (y * torch.from_numpy(w).to(dtype)).sum().backward()
            grads = {k: p.grad.numpy().copy() for k, p in named.items()}
            grads['x'] = xt.grad.numpy().copy()
            if mt is not None:
                grads['m'] = mt.grad.numpy().copy()
            return y.detach().numpy().copy(), [s.detach().numpy().copy() for s in states], grads

        y64, s64, g64 = run(torch.float64)
        y32, s32, g32 = run(torch.float32)
        devs = {'y': dev(y32, y64), **{f'out_state{i}': dev(a, c) for i, (a, c) in enumerate(zip(s32, s64))},
                **{'g_' + k: dev(g32[k], g64[k]) for k in g64}}
        zero = [k for k in g64 if np.abs(g64[k]).max() < 1e-12]
        ok = devs['y'] < VALUE / 4 and all(devs[f'out_state{i}'] < VALUE / 4 for i in range(len(s64))) \
            and all(devs['g_' + k] < GRAD / 4 for k in g64 if k not in zero)
        worst = max((k for k in g64 if k not in zero), key=lambda k: devs['g_' + k])
        print(f'{name:13s} seed {seed}: fp32 vs fp64 y {devs["y"]:.1e}, worst gradient {devs["g_" + worst]:.1e} ({worst}); '
              f'{len(zero)} analytically zero gradients')
        meta = dict(kw, state=bool(cfg.get('state')), seq_len=seq_len, seq_len_m=seq_len_m, keys=keys, names=list(g64), dev32=devs,
                    zero=zero, seed=seed)
        data = {f'{name}/x': x, f'{name}/w': w, f'{name}/y64': y64}
        if m is not None:
            data[f'{name}/m'] = m
        for i, s in enumerate(state or []):
            data[f'{name}/state{i}'] = s
        for i, s in enumerate(s64):
            data[f'{name}/out_state{i}'] = s
        for k, v in params.items():
            data[f'{name}/p_{k}'] = v
        for k, v in g64.items():
            data[f'{name}/g64_{k}'] = v
        return ok, meta, data

    seed = 2400
    while True:
        results = {name: run_variant(name, cfg, seed) for name, cfg in VARIANTS.items()}
        if all(ok for name, (ok, _, _) in results.items() if not name.startswith('batch')):
            break
        seed += 1

    index = dict(variants=np.array(json.dumps({name: meta for name, (_, meta, _) in results.items()})), seed=np.array(seed))
    for tq, tk in ((5, 9), (9, 5), (4, 4)):
        index[f'causal_{tq}_{tk}'] = get_causal_mask(torch.zeros(2, tq, tk, dtype=torch.float64)).numpy()
    rng = np.random.RandomState(seed)
    q, k, v = rng.randn(2, 2, 5, 4), rng.randn(2, 2, 9, 4), rng.randn(2, 2, 9, 6)
    mask = (rng.rand(2, 1, 5, 9) > 0.3).astype(np.float64)
    mask[:, :, :, 0] = 1                                           # (no row without a visible key)
    index.update(sdpa_q=q, sdpa_k=k, sdpa_v=v, sdpa_mask=mask)
    for label, kw in (('causal', dict(bidirectional=False)), ('lengths', dict(bidirectional=True, seq_len=[9, 3])),
                      ('causal_mask', dict(bidirectional=False, mask=torch.from_numpy(mask))),
                      ('lengths_mask', dict(bidirectional=True, seq_len=[9, 3], mask=torch.from_numpy(mask)))):
        out, weights = scaled_dot_product_attention(torch.from_numpy(q), torch.from_numpy(k), torch.from_numpy(v), **kw)
        index[f'sdpa_{label}_out'], index[f'sdpa_{label}_weights'] = out.numpy(), weights.numpy()
    path = HERE / 'g24_transformer.npz'
    np.savez_compressed(path, **index)
    print(path, path.stat().st_size, 'bytes')
    for name, (_, _, data) in results.items():
        path = HERE / f'g24_transformer_{name}.npz'
        np.savez_compressed(path, **data)
        print(path, path.stat().st_size, 'bytes')
        assert path.stat().st_size < (1 << 20), path


if __name__ == '__main__':
    main()
