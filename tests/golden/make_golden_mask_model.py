#!/usr/bin/env python3
"""Generate tests/golden/g19_mask_model.npz by importing the REAL reference's MaskEstimatorModel
(padertorch/contrib/jensheit/mask_estimator_example/model.py) around its MaskEstimator.

Run in the build container only (needs /root/reference):

    python tests/golden/make_golden_mask_model.py

The reference is imported exactly as make_golden_orpit.py does.  The output is data only.  Every case uses the tiny estimator of
tests/test_mask_estimator.py (hidden 8, fully connected [16, 12, 16], dropout 0); what differs is in CASES below:

    1     F 9, C 3, num_frames [7, 5, 4]   mean
    2     F 8, C 2, num_frames [6, 6]      median, power weights from a complex observation_stft
    3min  F 5, C 1, num_frames [4, 1]      min
    3max  the same                         max
    4     F 9, C 2, num_frames [5, 3]      mean, no noise target in the batch (the speech loss alone)

``inputs(case, seed)`` draws the observation's STFT (its magnitude is ``observation_abs``) and the mask targets (uniform in [0, 1]) from
a seeded numpy RandomState; they are stored as well.

Conditions, enforced by moving the seed and asserted at the end:
  * no input of a ReLU of the fp64 run lies within 1e-5 max|input| of zero (g15's tie margin);
  * for median, min and max the selected element's loss differs from its nearest unequal neighbour in sorted order by at least 1e-5 of
    its value (otherwise fp32 rounding would pick another element, which is not what is tested);
  * the reference's own fp32 run agrees with its fp64 run to half the tests' gates (values 1e-5 max|want|, gradients 2e-4 max|want|,
    loss scalars 1e-4 relative) in every stored quantity.

Keys per case ``<c>_``: ``seed``, ``margin`` (ReLU), ``gap`` (selection), ``keys`` / ``names`` (json: state_dict keys, named_parameters),
``p_<key>`` (state_dict), ``stft<b>`` complex64 ``[C, T_b, F]``, ``speech<b>`` / ``noise<b>`` the targets, ``out64_<key>`` / ``out32_<key>``
the padded outputs of the estimator, ``scalar_names`` (json, the review's scalars then ``loss``) with ``scalars64`` / ``scalars32``,
``single64`` [B] the review loss of every example alone, ``g64_<name>`` / ``g32_<name>`` the gradients of the review loss, ``review_keys`` (json).
"""
import json
import sys
from pathlib import Path

HERE = Path(__file__).resolve().parent
REPO = HERE.parent.parent

import numpy as np  # noqa: E402

CASES = {
    '1': dict(F=9, C=3, frames=[7, 5, 4], reduction='mean', stft=False, noise=True),
    '2': dict(F=8, C=2, frames=[6, 6], reduction='median', stft=True, noise=True),
    '3min': dict(F=5, C=1, frames=[4, 1], reduction='min', stft=False, noise=True),
    '3max': dict(F=5, C=1, frames=[4, 1], reduction='max', stft=False, noise=True),
    '4': dict(F=9, C=2, frames=[5, 3], reduction='mean', stft=False, noise=False),
}
TIE_MARGIN = 1e-5
GAP = 1e-5
VALUE, GRAD, SCALAR = 1e-5, 2e-4, 1e-4


def inputs(case, seed):
    """``(stft, speech, noise)``: per example complex64 ``[C, T_b, F]`` and two float32 targets in [0, 1]."""
    rng = np.random.RandomState(seed)
    stft, speech, noise = [], [], []
    for n in case['frames']:
        shape = (case['C'], n, case['F'])
        stft.append((rng.randn(*shape) + 1j * rng.randn(*shape)).astype(np.complex64))
        speech.append(rng.uniform(0, 1, size=shape).astype(np.float32))
        noise.append(rng.uniform(0, 1, size=shape).astype(np.float32))
    return stft, speech, noise


def build(case, seed):
    import torch
    from padertorch.contrib.jensheit.mask_estimator_example.model import MaskEstimatorModel  # the reference
    from padertorch.contrib.jensheit.mask_estimator_example.modul import MaskEstimator
    torch.manual_seed(seed)
    cfg = dict(num_features=case['F'])
    MaskEstimator.finalize_dogmatic_config(cfg)
    cfg['recurrent'].update(hidden_size=8)
    cfg['fully_connected'].update(hidden_size=[16, 12, 16], dropout=0., input_size=16)

    def make(node):
        if isinstance(node, dict) and 'factory' in node:
            return node['factory'](**{k: make(v) for k, v in node.items() if k != 'factory'})
        return node
    return MaskEstimatorModel(MaskEstimator(**{k: make(v) for k, v in cfg.items()}), reduction=case['reduction'])


def batch_of(case, seed, dtype, only=None):
    import torch
    stft, speech, noise = inputs(case, seed)
    pick = range(len(stft)) if only is None else [only]
    batch = dict(observation_abs=[torch.from_numpy(np.abs(stft[b])).to(dtype) for b in pick],
                 num_frames=[case['frames'][b] for b in pick],
                 speech_mask_target=[torch.from_numpy(speech[b]).to(dtype) for b in pick])
    if case['noise']:
        batch['noise_mask_target'] = [torch.from_numpy(noise[b]).to(dtype) for b in pick]
    if case['stft']:
        np_dtype = np.complex128 if dtype == torch.float64 else np.complex64
        batch['observation_stft'] = [stft[b].astype(np_dtype) for b in pick]
    return batch


def selection_gap(case, out, seed):
    """Smallest relative distance of a selected element's loss from its nearest unequal neighbour, over masks and examples."""
    if case['reduction'] == 'mean':
        return np.inf
    _, speech, noise = inputs(case, seed)
    gap = np.inf
    for key, targets in (('speech_mask_logits', speech), ('noise_mask_logits', noise)):
        for b, n in enumerate(case['frames']):
            x, t = out[key][b, :, :n].astype(np.float64).ravel(), targets[b].astype(np.float64).ravel()
            loss = np.sort(np.maximum(x, 0) - x * t + np.log1p(np.exp(-np.abs(x))))
            rank = dict(median=(loss.size - 1) // 2, min=0, max=loss.size - 1)[case['reduction']]
            others = loss[loss != loss[rank]]
            if others.size:
                gap = min(gap, float(np.abs(others - loss[rank]).min() / abs(loss[rank])))
    return gap


def run(net, case, seed, dtype, margins=None):
    import torch
    net = net.to(dtype)
    hooks = []
    if margins is not None:
        for m in net.modules():
            if isinstance(m, torch.nn.ReLU):
                hooks.append(m.register_forward_hook(
                    lambda _m, args, _out: margins.append(float(args[0].detach().abs().min() / args[0].detach().abs().max()))))
    batch = batch_of(case, seed, dtype)
    padded = net.estimator(batch['observation_abs'], batch['num_frames'])
    out = net(batch)
    for h in hooks:
        h.remove()
    review = net.review(batch, out)
    res = {'out_' + k: v.detach().numpy().copy() for k, v in padded.items()}
    scalar_names = list(review['scalars'])
    res['scalars'] = np.array([float(review['scalars'][k]) for k in scalar_names] + [float(review['loss'])])
    names = [n for n, _ in net.named_parameters()]
    for n, g in zip(names, torch.autograd.grad(review['loss'], [p for _, p in net.named_parameters()])):
        res['g_' + n] = g.numpy().copy()
    single = []
    for b in range(len(case['frames'])):
        one = batch_of(case, seed, dtype, only=b)
        single.append(float(net.review(one, net(one))['loss']))
    res['single'] = np.array(single)
    return res, dict(names=names, scalar_names=scalar_names + ['loss'], review_keys=list(review),
                     gap=selection_gap(case, {k[4:]: v for k, v in res.items() if k.startswith('out_')}, seed))


def ratios(r32, r64):
    """{quantity: |fp32 - fp64| / gate} of the reference's two runs."""
    out = {}
    for k, want in r64.items():
        err = np.abs(r32[k].astype(np.float64) - want)
        if k in ('scalars', 'single'):
            out[k] = float((err / np.abs(want)).max()) / SCALAR
            continue
        scale = float(np.abs(want).max())
        gate = GRAD if k.startswith('g_') else VALUE
        out[k] = float(err.max()) / (gate * scale) if scale > 0 else (0. if err.max() == 0 else float('inf'))
    return out


def main():
    sys.path[:0] = [str(HERE / 'ref_shim'), str(REPO), '/root/reference']
    import torch

    torch.set_num_threads(1)
    torch.use_deterministic_algorithms(True)
    out = {}
    for i, (c, case) in enumerate(CASES.items()):
        seed = 1900 + 100 * i
        while True:
            net = build(case, seed)
            params = {k: v.numpy().copy() for k, v in net.state_dict().items()}
            margins = []
            r64, info = run(net, case, seed, torch.float64, margins)
            if min(margins) >= TIE_MARGIN and info['gap'] >= GAP:
                r32, _ = run(build(case, seed), case, seed, torch.float32)
                rat = ratios(r32, r64)
                if max(rat.values()) <= 0.5:
                    break
                print(c, 'seed', seed, 'fp32 against fp64 above half a gate:', max(rat, key=rat.get), max(rat.values()), flush=True)
            else:
                print(c, 'seed', seed, 'refused: margin %.2e gap %.2e' % (min(margins), info['gap']), flush=True)
            seed += 1
        assert min(margins) >= TIE_MARGIN and info['gap'] >= GAP and max(rat.values()) <= 0.5
        p = c + '_'
        out[p + 'seed'], out[p + 'margin'], out[p + 'gap'] = np.array(seed), np.array(min(margins)), np.array(info['gap'])
        out[p + 'keys'] = np.array(json.dumps(list(params)))
        for k in ('names', 'scalar_names', 'review_keys'):
            out[p + k] = np.array(json.dumps(info[k]))
        for k, v in params.items():
            out[p + 'p_' + k] = v
        stft, speech, noise = inputs(case, seed)
        for b in range(len(case['frames'])):
            out[p + f'stft{b}'], out[p + f'speech{b}'], out[p + f'noise{b}'] = stft[b], speech[b], noise[b]
        for k in r64:
            head, _, tail = k.partition('_')
            if head in ('g', 'out'):
                out[p + head + '64_' + tail], out[p + head + '32_' + tail] = r64[k], r32[k]
            else:
                out[p + k + '64'], out[p + k + '32'] = r64[k], r32[k]
        print(c, 'seed', seed, 'margin %.2e' % min(margins), 'gap %.2e' % info['gap'], 'review', info['review_keys'], 'scalars',
              dict(zip(info['scalar_names'], r64['scalars'].round(4).tolist())),
              'worst fp32 vs fp64 share of a gate: %s %.3f' % (max(rat, key=rat.get), max(rat.values())))
    out['cases'] = np.array(json.dumps(CASES))
    path = HERE / 'g19_mask_model.npz'
    np.savez_compressed(path, **out)
    print(path, path.stat().st_size, 'bytes')


if __name__ == '__main__':
    main()
