#!/usr/bin/env python3
"""Time the One-and-Rest PIT model on the reference's ``convnet`` separator configuration (window 16, stride 8, 256 features,
``ConvNet(256, 8, 4, 512, 3, 'gLN')``) with ``flag_units = 20``, ``res-single``, ``K = 3`` targets (two iterations) at B = 4,
T = 32 000:

  * the whole step (forward + loss + backward), and
  * the loss + flag region alone (flag head, OR-PIT loss, flag loss; forward + backward on tensors of the model's shapes),

each on the HIP path (``ops.orpit``: csrc/orpit.hip) and on this script's own plain-torch restatement of the reference's loop
(``or_pit/model.py:187-218,319-379``: per example, per iteration, per candidate one ``log10(mean((e - t)^2))`` on slices, ``torch.min``,
a Python list of the targets left; ``rearrange`` + ``Linear`` + mean + sigmoid) on the same parameters and GPU in the same process.  The
separator is the HIP one in both chains.  It also reports the C-ABI calls of the region per iteration (from the script's own count of
``_lib.timed``) and the achieved HBM bandwidth of ``ptmi_td_rect_stats`` next to ``ptmi_td_pair_stats`` on the same number of bytes.

    python scripts/bench_orpit.py [--iters 10] [--warmup 3] [--rounds 5] [--out profiles/orpit.txt]

Method (scripts/bench_convnet.py): every chain is warmed up, then timed in ``rounds`` windows of ``iters`` iterations between two events,
the chains alternating window by window; reported are the median window (us per iteration) and min .. max.  Needs a GPU.
"""
import argparse
import json
import sys
from pathlib import Path

import torch
import torch.nn.functional as F

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
sys.path.insert(0, str(Path(__file__).resolve().parent))

from bench_convnet import measure, window  # noqa: E402

B, T, K, L, N, A = 4, 32000, 3, 16, 256, 20
HBM_GBS = 8000.     # MI355X peak HBM bandwidth, GB/s


def library_log_mse(e, t):
    return torch.log10(torch.mean((e - t) ** 2, dim=-1)).sum()


def library_one_and_rest(inputs, targets):
    """``or_pit/model.py:58-98`` with ``log_mse_loss`` and ``fill_missing_with_zeros=True``."""
    R = targets.shape[0]
    if R == 0:
        return library_log_mse(inputs, torch.zeros_like(inputs)), 0
    if R == 1:
        return library_log_mse(inputs, torch.cat([targets, torch.zeros_like(targets)], dim=0)), 0
    losses = [library_log_mse(inputs[0], targets[i]) + (1 / (R - 1)) * library_log_mse(
        inputs[1], torch.sum(targets[[j for j in range(R) if i != j]], dim=0)) for i in range(R)]
    return torch.min(torch.stack(losses), dim=0)


def library_loss(estimates, flags, s):
    """``or_pit/model.py:319-379``: the loop over examples and iterations, then the flag loss (``res-single``)."""
    reconstruction = 0
    for b in range(s.shape[0]):
        targets = s[b]
        for est in estimates:
            loss, perm = library_one_and_rest(est[b], targets)
            reconstruction = reconstruction + loss
            targets = targets[[i for i in range(targets.shape[0]) if i != perm]]      # (reads perm on the host, as the reference)
    total = reconstruction / s.shape[0]
    for k, flag in enumerate(flags):
        target = torch.ones_like(flag) if k == s.shape[1] - 2 else torch.zeros_like(flag)
        total = total + F.binary_cross_entropy(flag, target)
    return total


def library_flag(additional, flag_nn):
    pre = flag_nn(additional.transpose(1, 2))                                        # rearrange 'b o t -> b t o' + Linear
    return torch.sigmoid(torch.mean(pre, dim=(1, 2)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=10)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_orpit.py needs an MI355X'
    from padertorch_amd import _lib
    from padertorch_amd.contrib.examples.source_separation.or_pit import OneAndRestPIT
    from padertorch_amd.contrib.examples.source_separation.tasnet import TasDecoder, TasEncoder, TasNet
    from padertorch_amd.modules import ConvNet
    from padertorch_amd.ops import orpit
    dev = torch.device('cuda:0')
    torch.manual_seed(0)
    separator = TasNet(TasEncoder(L, N), ConvNet(N, 8, 4, 512, 3, 'gLN'), TasDecoder(L, N), num_speakers=2, additional_out_size=A)
    net = OneAndRestPIT(separator, finetune=True, flag_units=A).to(dev)
    params = list(net.parameters())
    s = torch.randn(B, K, T, device=dev) * torch.tensor([1.0, 0.6, 1.4], device=dev)[None, :, None]
    batch = dict(y=s.sum(1), s=s, num_samples=torch.full((B,), T, device=dev), num_speakers=[K] * B)
    lines = []

    def hip_step():
        loss = net.loss(batch, net(batch))['loss']
        return [loss.detach()] + list(torch.autograd.grad(loss, params))

    def library_step():
        outs = net(batch)['outs']
        flags = [library_flag(o['additional_out'], net.flag_nn) for o in outs]
        loss = library_loss([o['out'] for o in outs], flags, s)
        return [loss.detach()] + list(torch.autograd.grad(loss, params))
    worst = max(float((p - q).abs().max() / q.abs().max().clamp(min=1e-30)) for p, q in zip(hip_step(), library_step()))
    lines.append(f'# loss and parameter gradients of the two chains differ by at most {worst:.1e} of their maximum')
    print(lines[-1], flush=True)
    assert worst <= 5e-2, worst
    lines.append(measure(f'OneAndRestPIT (convnet separator, flag_units {A}, res-single, K {K}: two iterations) B={B} T={T}, forward + '
                         'loss + backward', dict(hip=hip_step, library=library_step), args))

    # the loss + flag region alone
    E = T // (L // 2) - 1
    ests = [torch.randn(B, 2, T, device=dev, requires_grad=True) for _ in range(K - 1)]
    adds = [torch.randn(B, A, E, device=dev, requires_grad=True) for _ in range(K - 1)]
    leaves = ests + adds + list(net.flag_nn.parameters())

    def hip_region():
        flags = [orpit.flag_head(a, net.flag_nn.weight, net.flag_nn.bias)[0] for a in adds]
        loss = net.loss(batch, dict(outs=[dict(out=e, flag=f) for e, f in zip(ests, flags)]))['loss']
        return [loss.detach()] + list(torch.autograd.grad(loss, leaves))

    def library_region():
        loss = library_loss(ests, [library_flag(a, net.flag_nn) for a in adds], s)
        return [loss.detach()] + list(torch.autograd.grad(loss, leaves))
    worst = max(float((p - q).abs().max() / q.abs().max().clamp(min=1e-30)) for p, q in zip(hip_region(), library_region()))
    assert worst <= 1e-3, worst
    _lib.KERNEL_TIMERS = []
    hip_region()
    torch.cuda.synchronize()
    calls = [name for name, _, _ in _lib.KERNEL_TIMERS]
    _lib.KERNEL_TIMERS = None
    count = {n: calls.count(n) for n in dict.fromkeys(calls)}
    lines.append(measure(f'loss + flag region (flag head, OR-PIT loss, flag loss) B={B} T={T} E={E}, {K - 1} iterations, forward + backward',
                         dict(hip=hip_region, library=library_region), args,
                         extra=lambda res: dict(c_abi_calls=count, c_abi_calls_per_iteration=len(calls) / (K - 1))))

    # the statistics kernel against ptmi_td_pair_stats on the same bytes: (2 + 3) rows of 32 000 = (2 + 2) rows of 40 000 samples
    lib = _lib.load()
    est, tgt = ests[0].detach(), s
    e2, t2 = torch.randn(B, 2, 5 * T // 4, device=dev), torch.randn(B, 2, 5 * T // 4, device=dev)
    stats = torch.empty((B, int(lib.ptmi_td_stats_elems(2))), dtype=torch.float64, device=dev)
    ws = torch.empty(int(lib.ptmi_td_workspace_elems(B, 2, e2.shape[2])), dtype=torch.float64, device=dev)
    strides = _lib.int64s(e2.stride(0), e2.stride(1), t2.stride(0), t2.stride(1))

    def rect():
        torch.ops.ptmi.td_rect_stats(est, tgt, True)

    def pair():
        _lib.check(lib.ptmi_td_pair_stats(e2.data_ptr(), t2.data_ptr(), None, B, 2, e2.shape[2], strides, ws.data_ptr(), stats.data_ptr(),
                                          _lib.stream(dev)), 'ptmi_td_pair_stats')
    nbytes = B * 5 * T * 4
    for fn in (rect, pair):
        for _ in range(5):
            fn()
    res = {}
    for name, fn in (('td_rect_stats', rect), ('td_pair_stats', pair)):
        us = sorted(window(fn, 50) for _ in range(args.rounds))[args.rounds // 2]
        res[name] = dict(median_us=round(us, 2), gb_per_s=round(nbytes / us / 1e3, 1), hbm_fraction=round(nbytes / us / 1e3 / HBM_GBS, 4))
    lines.append(json.dumps(dict(what=f'statistics pass, both launches of each call, {nbytes} bytes read (B={B}: 2 + {K} rows of {T} against '
                                      f'2 + 2 rows of {5 * T // 4}); td_rect_stats with the Gram matrix', **res)))
    print(lines[-1], flush=True)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
