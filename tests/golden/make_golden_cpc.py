#!/usr/bin/env python3
"""Generate tests/golden/g30_cpc.npz from the REAL reference's ``CPC1d`` (padertorch/contrib/mk/modules/contrastive.py) on the CPU.

Run in the build container only (needs /root/reference):

    python tests/golden/make_golden_cpc.py

The reference is imported exactly as make_golden_je_conv.py does (plus a ``torchvision.utils`` stand-in under ref_shim).  The output is
data only.  Encoder ``CNN1d(6, [8, 8], 3)``, both heads ``CNN1d(8, [8, 16], 1)`` (two steps of 8 features each), ``feature_extractor=None``,
``x [3, 6, 40]`` with lengths ``[40, 33, 25]``, steps ``fwd (2, 5)`` / ``bwd (-3, -1)``, temperature 2.  ``CASES`` lists the three
configurations.  Keys: ``x``, ``seq_len``, ``labels``, ``keys`` (json: parameter names), and per case ``<c>_p_<name>`` (parameters),
``<c>_logits<i>`` (fp64, per step), ``<c>_ce``, ``<c>_scalars`` (json order ``<c>_scalar_names``), ``<c>_g_<name>`` (fp64 gradients of the
encoder's parameters) and ``<c>_d32`` = the reference's own fp32-vs-fp64 differences ``[ce, scalars, logits, gradients]``, each relative
to the largest fp64 magnitude of the quantity; the test gates at four times these.
"""
import json
import sys
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
REPO = HERE.parent.parent

B, C, T, D = 3, 6, 40, 8
LENGTHS = [40, 33, 25]
LABELS = [0, 1, 0]
STEPS = dict(fwd_prediction_steps=(2, 5), bwd_prediction_steps=(-3, -1))
CASES = {
    'time': dict(negatives_mode='time', negative_to_target_dist=3, l2_normalization=True),
    'all': dict(negatives_mode='all', l2_normalization=False, multi_view=False),
    'batch': dict(negatives_mode='batch', batch_mask_key='labels'),
}


def build(cls, cnn, case, dtype, **extra):
    import torch
    torch.manual_seed(3000 + sorted(CASES).index(case))
    model = cls(cnn(C, [D, D], 3), cnn(D, [D, 2 * D], 1), cnn(D, [D, 2 * D], 1), None, temperature=2., input_key='x',
                input_seq_len_key='seq_len', **STEPS, **CASES[case], **extra)
    return model.to(dtype)


def inputs():
    rng = np.random.RandomState(30)
    return rng.randn(B, C, T).astype(np.float32)


def run(model, dtype):
    import torch
    batch = dict(x=torch.from_numpy(inputs()).to(dtype), seq_len=list(LENGTHS), labels=np.array(LABELS))
    outputs = model(batch)
    review = model.review(batch, outputs)
    ce = review['losses']['ce']
    named = [(n, p) for n, p in model.named_parameters() if n.startswith('encoder.')]
    grads = torch.autograd.grad(ce, [p for _, p in named])
    scalars = {k: float(v) for k, v in review['scalars'].items()}
    return dict(logits=[l.detach().numpy() for l in outputs[0]], ce=float(ce), scalars=scalars,
                grads={n: g.numpy() for (n, _), g in zip(named, grads)})


def main():
    sys.path[:0] = [str(HERE / 'ref_shim'), str(REPO), '/root/reference']
    import torch
    from padertorch.contrib.je.modules.conv import CNN1d
    from padertorch.contrib.mk.modules.contrastive import CPC1d
    out = dict(x=inputs(), seq_len=np.array(LENGTHS), labels=np.array(LABELS))
    for case in CASES:
        model = build(CPC1d, CNN1d, case, torch.float64)
        r64 = run(model, torch.float64)
        r32 = run(build(CPC1d, CNN1d, case, torch.float32), torch.float32)
        for n, p in model.state_dict().items():
            out[f'{case}_p_{n}'] = p.numpy()
        out['keys'] = json.dumps(list(model.state_dict()))
        for i, l in enumerate(r64['logits']):
            out[f'{case}_logits{i}'] = l
        out[f'{case}_ce'] = np.array(r64['ce'])
        out[f'{case}_scalar_names'] = json.dumps(list(r64['scalars']))
        out[f'{case}_scalars'] = np.array(list(r64['scalars'].values()))
        for n, g in r64['grads'].items():
            out[f'{case}_g_{n}'] = g
        fin = [np.isfinite(l) for l in r64['logits']]
        top = max(np.abs(l[f]).max() for l, f in zip(r64['logits'], fin))
        d32 = [abs(r32['ce'] - r64['ce']) / abs(r64['ce']),
               max(abs(r32['scalars'][k] - v) / max(abs(v), 1e-30) for k, v in r64['scalars'].items()),
               max(np.abs(a[f].astype(np.float64) - l[f]).max() for a, l, f in zip(r32['logits'], r64['logits'], fin)) / top,
               max(np.abs(r32['grads'][n].astype(np.float64) - g).max() / np.abs(g).max() for n, g in r64['grads'].items())]
        out[f'{case}_d32'] = np.array(d32)
        print(case, 'ce', r64['ce'], 'fp32 vs fp64 [ce, scalars, logits, gradients]:', d32, r64['scalars'])
    np.savez_compressed(HERE / 'g30_cpc.npz', **out)


if __name__ == '__main__':
    main()
