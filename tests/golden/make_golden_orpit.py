#!/usr/bin/env python3
"""Generate tests/golden/g16_orpit.npz by importing the REAL reference's OneAndRestPIT (padertorch/contrib/examples/source_separation/
or_pit/model.py) on its TasNet, TasEncoder, TasDecoder and ConvNet.

Run in the build container only (needs /root/reference):

    python tests/golden/make_golden_orpit.py

The reference is imported exactly as make_golden_tasnet.py does.  The output is data only.  Every case uses TasEncoder(16, 12),
ConvNet(8, 2, 1, 16, 3), sigmoid masks and T = 208 (26 half windows: no padding); what differs is in CASES below:

    a  K 2, res-single, mean, B 3                                          one iteration
    b  K 3, res-silent, res-weighted-mean, gradients between iterations, cLN    three iterations; also a second batch (``alt``) on which
                                                                           the reference chooses the targets in ANOTHER order
    c  K 4, est-silent, est-weighted-mean                                  four iterations (max_iterations), three estimates
    d  K 3, no flag (flag_units 0), stop_condition 'none'                  two iterations
    e  K 3, finetune=False                                                 one iteration whatever K is
    f  K 2, separator with mask=False, res-weighted-mean                   the mask IS the estimate

``inputs(case, seed)`` draws the mixtures ``y [B, T]`` and the targets ``s [B, K, T]`` (each at its own level) from a seeded numpy RandomState; they are NOT stored,
the tests call the same function.  The parameters of norms and PReLUs are redrawn as in g15, the output projection's weight from [-1, 1].

Conditions, enforced by moving the seed:
  * no input of a ReLU / PReLU of the fp64 run lies within 1e-5 max|input| of zero (g15's tie margin);
  * wherever two or more candidate targets compete, the best and the second best loss differ by at least 1e-3 (a tie flip would change
    the target order, which is not what is tested), and a flag that decides ``decode`` is at least 1e-3 from the threshold;
  * the reference's own fp32 run agrees with its fp64 run to half the tests' gates (values 1e-5 max|want|, gradients 2e-4 max|want|,
    loss scalars 1e-4) in every stored quantity, and chooses the same targets.

Keys per case ``<c>_``: ``seed``, ``margin`` (ReLU), ``gap`` (candidates), ``keys`` / ``names`` (json: state_dict keys, named_parameters),
``p_<key>``, ``out64`` / ``out32``, per iteration ``it<k>_out64`` / ``_flag64`` / ``_pre64`` (and 32), ``order`` [B, iterations] (indices into
the targets), ``scalar_names`` (json) with ``scalars64`` / ``scalars32``, ``g64_<name>`` / ``g32_<name>`` the gradients of the review loss,
``review_keys`` (json), ``decode_iterations`` (decode on the first example alone, max_iterations 4).  ``b_alt_seed`` / ``b_alt_order`` /
``b_alt_loss64``: the second batch of case b.
``fn_*``: ``one_and_rest_permutation_invariant_loss`` on ``fn_inputs(K, T)`` for K 0..4, T in {1, 57}, both values of
``fill_missing_with_zeros``, with ``log_mse_loss`` and ``mse_loss``: ``fn_<loss>_K<K>_T<T>_<fill>`` = [loss, perm] (fp64).
"""
import json
import sys
from pathlib import Path

HERE = Path(__file__).resolve().parent
REPO = HERE.parent.parent

import numpy as np  # noqa: E402

T = 208
BASE = dict(B=2, norm='gLN', unroll_type='res-single', flag_reduction='mean', flag_units=5, stop_condition='flag', finetune=True,
            propagate=False, mask=True)
CASES = {
    'a': dict(BASE, K=2, B=3),
    'b': dict(BASE, K=3, unroll_type='res-silent', flag_reduction='res-weighted-mean', propagate=True, norm='cLN'),
    'c': dict(BASE, K=4, unroll_type='est-silent', flag_reduction='est-weighted-mean'),
    'd': dict(BASE, K=3, flag_units=0, stop_condition='none'),
    'e': dict(BASE, K=3, finetune=False),
    'f': dict(BASE, K=2, mask=False, flag_reduction='res-weighted-mean'),
}
TIE_MARGIN = 1e-5
GAP = 1e-3
VALUE, GRAD, SCALAR = 1e-5, 2e-4, 1e-4
FN_LOSSES = ['log_mse_loss', 'mse_loss']


def inputs(case, seed):
    """``(y [B, T], s [B, K, T])``, float32: every target has a level of its own in [0.5, 1.5], so that the candidates differ, and the
    mixture is their sum (fp32) plus a little noise."""
    rng = np.random.RandomState(seed)
    B, K = case['B'], case['K']
    noise, s, level = rng.randn(B, T), rng.randn(B, K, T), rng.uniform(0.5, 1.5, size=(B, K, 1))
    s = (s * level).astype(np.float32)
    return s.sum(1) + (0.1 * noise).astype(np.float32), s


def fn_inputs(K, length):
    """``(inputs [2, length], targets [K, length])``, float32, for the loss function alone."""
    rng = np.random.RandomState(1600 + 10 * K + length)
    return rng.randn(2, length).astype(np.float32), rng.randn(K, length).astype(np.float32)


def parameter_range(name):
    """The range a parameter is redrawn from, or None to keep its initialisation (as make_golden_tasnet.py)."""
    leaf = name.rsplit('.', 1)[1]
    if name.endswith('output_proj.weight'):     # masks away from 1/2: an untrained separator would give two equal outputs, and
        return -1., 1.                          # with them two equal candidates in every iteration
    if name.endswith(('encoder_1d.weight', 'decoder_1d.weight')):       # a gain near one from pass to pass: the initialisation's would
        return -0.5, 0.5                                                # let the residual fade, and the candidates with it
    if 'activation_fn' in name or 'output_prelu' in name or 'output_nonlinearity' in name:
        return 0.1, 0.4
    if '.conv.' not in name and 'norm' in name and leaf in ('gamma', 'weight'):
        return 0.5, 1.5
    if '.conv.' not in name and 'norm' in name and leaf in ('beta', 'bias'):
        return -0.5, 0.5
    return None


def build(case, seed):
    import torch
    from padertorch.contrib.examples.source_separation.or_pit.model import OneAndRestPIT  # the reference
    from padertorch.contrib.examples.source_separation.tasnet.model import TasNet
    from padertorch.contrib.examples.source_separation.tasnet.tas_coders import TasDecoder, TasEncoder
    from padertorch.modules.convnet import ConvNet
    torch.manual_seed(seed)
    separator = TasNet(TasEncoder(16, 12), ConvNet(input_size=8, num_blocks=2, num_repeats=1, hidden_channels=16, kernel_size=3,
                                                   norm=case['norm']),
                       TasDecoder(16, 12), mask=case['mask'], num_speakers=2, additional_out_size=case['flag_units'])
    net = OneAndRestPIT(separator, finetune=case['finetune'], unroll_type=case['unroll_type'], stop_condition=case['stop_condition'],
                        propagate_grad_between_iterations=case['propagate'], flag_reduction=case['flag_reduction'],
                        flag_units=case['flag_units'])
    rng = np.random.RandomState(seed + 1)
    with torch.no_grad():
        for name, p in net.named_parameters():
            span = parameter_range(name)
            if span is not None:
                p.copy_(torch.from_numpy(rng.uniform(*span, size=tuple(p.shape)).astype(np.float32)))
    return net


def candidate_gaps(outs, s):
    """The reference's loop over examples and iterations restated in numpy: the chosen order [B, iterations] and the smallest
    difference between the best and the second best candidate."""
    order, gap = [], np.inf
    for b in range(s.shape[0]):
        left, row = list(range(s.shape[1])), []
        for o in outs:
            e = o[b].astype(np.float64)
            if len(left) >= 2:
                cand = []
                for i in left:
                    rest = s[b, [j for j in left if j != i]].astype(np.float64).sum(0)
                    cand.append(np.log10(np.mean((e[0] - s[b, i]) ** 2)) + np.log10(np.mean((e[1] - rest) ** 2)) / (len(left) - 1))
                best = int(np.argmin(cand))
                gap = min(gap, float(np.sort(cand)[1] - np.sort(cand)[0]))
            else:
                best = 0
            row.append(left.pop(best))
        order.append(row)
    return np.array(order, dtype=np.int64), gap


def run(net, case, seed, dtype, margins=None, grads=True):
    import torch
    y0, s0 = inputs(case, seed)
    net = net.to(dtype)
    hooks = []
    if margins is not None:
        def margin_of(t):
            margins.append(float(t.detach().abs().min() / t.detach().abs().max()))
        hooks.append(net.separator.encoder.encoder_1d.register_forward_hook(lambda _m, _args, out: margin_of(out)))
        for m in net.modules():
            if isinstance(m, (torch.nn.PReLU, torch.nn.ReLU)):
                hooks.append(m.register_forward_hook(lambda _m, args, _out: margin_of(args[0])))
    B, K = case['B'], case['K']
    batch = dict(y=list(torch.from_numpy(y0).to(dtype)), s=list(torch.from_numpy(s0).to(dtype)), num_samples=[T] * B, num_speakers=[K] * B)
    out = net(batch)
    for h in hooks:
        h.remove()
    review = net.review(batch, out)
    res = dict(out=out['out'].detach().numpy().copy())
    for k, o in enumerate(out['outs']):
        res[f'it{k}_out'] = o['out'].detach().numpy().copy()
        if case['flag_units']:
            res[f'it{k}_flag'] = o['flag'].detach().numpy().copy()
            res[f'it{k}_pre'] = o['pre_mean_flag'].detach().numpy().copy()
    scalar_names = list(review['scalars'])
    res['scalars'] = np.array([float(review['scalars'][k]) for k in scalar_names] + [float(review['loss'])])
    names = [n for n, _ in net.named_parameters()]
    if grads:
        for n, g in zip(names, torch.autograd.grad(review['loss'], [p for _, p in net.named_parameters()])):
            res['g_' + n] = g.numpy().copy()
    order, gap = candidate_gaps([o['out'].detach().numpy() for o in out['outs']], s0)
    return res, dict(names=names, scalar_names=scalar_names + ['loss'], review_keys=list(review), order=order, gap=gap)


def decode_count(net, case, seed, dtype):
    """Iterations ``decode`` runs on the first example alone, and the smallest distance of a deciding flag from the threshold."""
    import torch
    y0, _ = inputs(case, seed)
    net = net.to(dtype)
    with torch.no_grad():
        out = net.decode(dict(y=[torch.from_numpy(y0[0]).to(dtype)], num_samples=[T]), max_iterations=4)
    distance = min((abs(float(o['flag']) - net.threshold) for o in out['outs']), default=np.inf) if case['stop_condition'] == 'flag' else np.inf
    return len(out['outs']), distance


def ratios(r32, r64):
    """{quantity: |fp32 - fp64| / gate} of the reference's two runs (the gate relative to max|fp64|, absolute for the scalars)."""
    out = {}
    for k, want in r64.items():
        err = float(np.abs(r32[k].astype(np.float64) - want).max())
        if k == 'scalars':
            out[k] = err / SCALAR
            continue
        scale = float(np.abs(want).max())
        gate = GRAD if k.startswith('g_') else VALUE
        out[k] = err / (gate * scale) if scale > 0 else (0. if err == 0 else float('inf'))
    return out


def main():
    sys.path[:0] = [str(HERE / 'ref_shim'), str(REPO), '/root/reference']
    import torch
    import padertorch as pt
    from padertorch.contrib.examples.source_separation.or_pit.model import one_and_rest_permutation_invariant_loss

    torch.set_num_threads(1)
    torch.use_deterministic_algorithms(True)
    out = {}
    for i, (c, case) in enumerate(CASES.items()):
        seed = 1600 + 100 * i
        while True:
            net = build(case, seed)
            params = {k: v.numpy().copy() for k, v in net.state_dict().items()}
            margins = []
            r64, info = run(net, case, seed, torch.float64, margins)
            count, distance = decode_count(build(case, seed), case, seed, torch.float64)
            if min(margins) >= TIE_MARGIN and info['gap'] >= GAP and distance >= GAP:
                r32, info32 = run(build(case, seed), case, seed, torch.float32)
                rat = ratios(r32, r64)
                count32, _ = decode_count(build(case, seed), case, seed, torch.float32)
                if max(rat.values()) <= 0.5 and np.array_equal(info['order'], info32['order']) and count == count32:
                    break
                print(c, 'seed', seed, 'fp32 against fp64 above half a gate:', max(rat, key=rat.get), max(rat.values()),
                      'orders equal', np.array_equal(info['order'], info32['order']), 'decode', count, count32, flush=True)
            else:
                print(c, 'seed', seed, 'refused: margin %.2e gap %.2e flag distance %.2e' % (min(margins), info['gap'], distance), flush=True)
            seed += 1
        p = c + '_'
        out[p + 'seed'], out[p + 'margin'], out[p + 'gap'] = np.array(seed), np.array(min(margins)), np.array(info['gap'])
        out[p + 'keys'] = np.array(json.dumps(list(params)))
        for k in ('names', 'scalar_names', 'review_keys'):
            out[p + k] = np.array(json.dumps(info[k]))
        for k, v in params.items():
            out[p + 'p_' + k] = v
        out[p + 'order'], out[p + 'decode_iterations'] = info['order'], np.array(count)
        for k in r64:
            head, _, tail = k.partition('_')
            if head == 'g':
                out[p + 'g64_' + tail], out[p + 'g32_' + tail] = r64[k], r32[k]
            else:
                out[p + k + '64'], out[p + k + '32'] = r64[k], r32[k]
        print(c, 'seed', seed, 'margin %.2e' % min(margins), 'gap %.2e' % info['gap'], 'iterations', info['order'].shape[1], 'order',
              info['order'].tolist(), 'decode', count, 'worst fp32 vs fp64 share of a gate: %s %.3f' % (max(rat, key=rat.get), max(rat.values())))
        if c == 'b':            # a second batch on which the targets come in another order (the captured step replays both)
            alt = seed + 1000
            while True:
                r, alt_info = run(build(case, seed), case, alt, torch.float64, grads=False)
                r32, alt32 = run(build(case, seed), case, alt, torch.float32, grads=False)
                if alt_info['gap'] >= GAP and not np.array_equal(alt_info['order'], info['order']) \
                        and np.array_equal(alt_info['order'], alt32['order']):
                    break
                alt += 1
            out['b_alt_seed'], out['b_alt_order'], out['b_alt_loss64'] = np.array(alt), alt_info['order'], r['scalars'][-1:]
            print('b alt seed', alt, 'order', alt_info['order'].tolist())
    fns = {'log_mse_loss': pt.log_mse_loss, 'mse_loss': pt.mse_loss}
    for name in FN_LOSSES:
        for K in range(5):
            for length in (1, 57):
                for fill in (False, True):
                    x, t = (torch.from_numpy(a).double() for a in fn_inputs(K, length))
                    loss, perm = one_and_rest_permutation_invariant_loss(x, t, fns[name], fill_missing_with_zeros=fill)
                    out[f'fn_{name}_K{K}_T{length}_{int(fill)}'] = np.array([float(loss), float(perm)])
    out['cases'] = np.array(json.dumps(CASES))
    path = HERE / 'g16_orpit.npz'
    np.savez_compressed(path, **out)
    print(path, path.stat().st_size, 'bytes')


if __name__ == '__main__':
    main()
