#!/usr/bin/env python3
"""Generate tests/golden/g29_je_features.npz from the REAL reference's NormalizedLogMelExtractor (imported through ref_shim), on the CPU,
seeded, in float64 and in float32: ``python tests/golden/make_golden_je_features.py`` (needs the reference tree; build container only).

Data only: outputs, returned seq_len and targets, the norm's buffers and the drawn tables (a test failure on them reads "stream order",
not "kernel").  Inputs come from ``inputs``, which the test calls too.  Adjusted inside this process only: ``np.int`` is aliased to
``int``; the blur's sigma sampler (paderbox's, which the shim does not sample) is replaced by ``sigma_fn`` on the instance, as the test
does on ours; for the float64 run ``conv2d`` casts the float32 blur kernel to the input's type.

Cases (STFT size 64 at 16 kHz, 10 filters, ``B = 4``, ``T = 40``, ragged): c0 evaluation, defaults; c1 training with both deltas, two
successive batches (``c1a``, ``c1b``) and the norm's buffers after each; c2 two channels with ``ipd_pairs = ((0, 1),)``; c3 training
with scale, superposition, time warping, blur, mixup, two time masks and a frequency mask, with targets.  The generator refuses to write
when the reference's own float32 run is further than a quarter of a case's gate from its float64 run.
"""
import sys
from pathlib import Path
from types import SimpleNamespace

import numpy as np

HERE = Path(__file__).resolve().parent
REPO = HERE.parent.parent
B, T, LENGTHS, SEED = 4, 40, [40, 33, 21, 9], 2900
BASE = dict(sample_rate=16000, stft_size=64, number_of_filters=10)
#: per case: four times the largest |float32 run - float64 run| of the reference's output (measured, printed below: 2.04e-7, 1.78e-6,
#: 1.73e-7, 5.6e-7) - the gates of test_gpu_je_features.py on max |ours - float64 run|
GATES = {'c0': 8.2e-7, 'c1': 7.2e-6, 'c2': 7.0e-7, 'c3': 2.3e-6}


def scale_fn(n):
    return np.random.uniform(.5, 2., n)


def sigma_fn(n):
    return .1 + np.minimum(np.random.exponential(.5, n), 5.)


def time_warp(seq_len):
    seq_len = np.asarray(seq_len)
    factor = np.random.uniform(.8, 1.25, len(seq_len))
    return np.minimum(np.arange(max(seq_len))[None] / factor[:, None], max(seq_len) - 1), np.minimum(factor * seq_len, max(seq_len))


CASES = {
    'c0': (False, dict()),
    'c1': (True, dict(add_deltas=True, add_delta_deltas=True)),
    'c2': (False, dict(num_channels=2, ipd_pairs=((0, 1),))),
    'c3': (True, dict(scale_sampling_fn=scale_fn, superposition_prob=.5, time_warping_fn=time_warp, blur_sigma=.5, mixup_prob=.5,
                      n_time_masks=2, max_masked_time_steps=12, n_frequency_masks=1, max_masked_frequency_bands=4)),
}


def inputs(case, batch=0):
    """``(x [B, C, T, 33, 2] float32, zero behind each row's length; targets [B, 5] float32)``."""
    rng = np.random.RandomState(SEED + 10 * int(case[1]) + batch)
    x = rng.randn(B, CASES[case][1].get('num_channels', 1), T, 33, 2).astype(np.float32)
    for b, n in enumerate(LENGTHS):
        x[b, :, n:] = 0.
    return x, (rng.rand(B, 5) > .6).astype(np.float32)


def run(cls, case, dtype, device='cpu', prepare=None):
    """One seeded pass of ``cls`` over the case's batches -> ``{key: array}``; ``prepare(module)`` adjusts the fresh instance."""
    import torch
    training, kw = CASES[case]
    ext = cls(**BASE, **kw).train(training)
    if ext.blur is not None:
        ext.blur.sigma_sampling_fn = sigma_fn
    if prepare is not None:
        prepare(ext)
    ext = ext.to(dtype).to(device)
    np.random.seed(SEED)
    torch.manual_seed(SEED)
    out = {}
    for i, tag in enumerate(('a', 'b') if case == 'c1' else ('',)):
        x, targets = inputs(case, i)
        res = ext(torch.from_numpy(x).to(dtype).to(device), list(LENGTHS), torch.from_numpy(targets).to(device) if case == 'c3' else None)
        out[case + tag + '_y'] = res[0].double().cpu().numpy()
        out[case + tag + '_seq_len'] = np.asarray(res[1], dtype=np.float64)
        if len(res) > 2:
            out[case + tag + '_targets'] = res[2].double().cpu().numpy()
        for name in ('num_tracked_values', 'running_mean', 'running_power'):
            out[case + tag + '_' + name] = getattr(ext.norm, name).double().cpu().numpy().copy()
    return out


def draws():
    """The tables c3 draws, in the order of ``forward``: the same calls on the same seeds."""
    import torch
    np.random.seed(SEED)
    torch.manual_seed(SEED)
    host = np.concatenate([[np.random.choice(B - 1)], np.random.binomial(1, .5, B), scale_fn(B), scale_fn(B), np.random.uniform(.8, 1.25, B),
                           sigma_fn(B), [np.random.choice(B)], np.random.binomial(1, .5, B), np.random.beta(1., 1., B)])
    return host, np.stack([torch.rand(B).numpy() for _ in range(6)])


def main():
    sys.path[:0] = [str(HERE / 'ref_shim'), str(REPO), '/root/reference']
    np.int = int
    import torch
    from padertorch.contrib.je.modules import augment as ref_augment
    from padertorch.contrib.je.modules.features import NormalizedLogMelExtractor

    fn = torch.nn.functional
    ref_augment.F = SimpleNamespace(pad=fn.pad, conv2d=lambda x, kernel, **kw: fn.conv2d(x, kernel.to(x.dtype), **kw))
    torch.set_num_threads(1)
    out = {}
    for case in CASES:
        r64, r32 = run(NormalizedLogMelExtractor, case, torch.float64), run(NormalizedLogMelExtractor, case, torch.float32)
        for k in r64:
            err = float(np.abs(r64[k] - r32[k]).max())
            if k.endswith('_y'):
                print(k, r64[k].shape, 'float32 run off by %.3g' % err)
                assert err <= GATES[case] / 4, f'{k}: the reference\'s float32 run is more than a quarter of the gate {GATES[case]} from its float64 run'
            else:
                assert err <= 1e-4 * max(1., float(np.abs(r64[k]).max())), (k, err)
        out.update(r64)
    out['c3_draws_np'], out['c3_draws_torch'] = draws()
    path = HERE / 'g29_je_features.npz'
    np.savez_compressed(path, **out)
    print(path, path.stat().st_size, 'bytes')


if __name__ == '__main__':
    main()
