#!/usr/bin/env python3
"""Time the WaveNet vocoder (csrc/wavenet.hip, ops/wavenet.py) beside the same arithmetic through torch's own operators on the same GPU.

    python scripts/bench_wavenet.py [--window 0.5] [--rounds 3] [--out profiles/wavenet.txt]

Net: R = 64 residual, S = 256 skip, A = 256 classes, L = 16 layers (max_dilation 128), 80 conditioning channels, window 1024, stride 256.

    training   forward + backward of sum(output * w), B = 4, T = 16000: ``modules.WaveNet`` against the reference's formulation in
               F.conv_transpose1d / F.conv1d (``[B, C, T]``, autograd's backward).  Alternating windows of at least ``--window`` seconds
               between device events, ``--rounds`` rounds, median.
    sampling   ``ops.wavenet.generate`` at 1, 4 and 16 sequences over ``--steps`` time steps (one timing per launch configuration, device
               events around all launches), against a per-step loop of torch operators over ``--torch-steps`` steps.  ``us_per_step`` of one
               workgroup gives the steps a launch may cover to stay near 100 ms (``steps_for_100ms``): what ``STEPS_PER_LAUNCH`` is set from.

Recorded, not gated.  One JSON line per measurement.  Needs a GPU.
"""
import argparse
import json
import statistics
import sys
from pathlib import Path

import torch
import torch.nn.functional as F

REPO = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(REPO), str(REPO / 'tests')]

NET = dict(n_cond_channels=80, upsamp_window=1024, upsamp_stride=256, n_in_channels=256, n_layers=16, max_dilation=128,
           n_residual_channels=64, n_skip_channels=256, n_out_channels=256, fading='full')


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e-3 / reps


def torch_forward(m, features, audio):
    """WaveNet.forward through torch's operators (``[B, C, T]``; cond_layers applied once)."""
    from padertorch_amd.ops import wavenet as wn
    R, L = m.n_residual_channels, m.n_layers
    with torch.no_grad():
        quantized = torch.ops.ptmi.mu_law_encode(audio, m.n_in_channels)
    T = quantized.shape[1]
    front, back = wn.crop_of(m.fading, m.upsamp_window, m.upsamp_stride)
    up = F.conv_transpose1d(features, m.upsample.weight, m.upsample.bias, stride=m.upsamp_stride)
    up = up[..., front:up.shape[-1] - back][..., :T]
    cond = F.conv1d(up, m.cond_layers.conv.weight, m.cond_layers.conv.bias)
    x = F.embedding(quantized, m.embed.weight).transpose(1, 2)
    skip = None
    for l, d in enumerate(m.dilations):
        conv = m.dilate_layers[l].conv
        z = F.conv1d(F.pad(x, (d, 0)), conv.weight, conv.bias, dilation=d) + cond[:, l * 2 * R:(l + 1) * 2 * R]
        acts = torch.tanh(z[:, :R]) * torch.sigmoid(z[:, R:])
        s = F.conv1d(acts, m.skip_layers[l].conv.weight, m.skip_layers[l].conv.bias)
        skip = s if skip is None else skip + s
        if l < L - 1:
            x = x + F.conv1d(acts, m.res_layers[l].conv.weight, m.res_layers[l].conv.bias)
    out = F.conv1d(torch.relu(F.conv1d(torch.relu(skip), m.conv_out.conv.weight)), m.conv_end.conv.weight)
    return torch.cat((torch.zeros_like(out[..., :1]), out[..., :-1]), -1)


def torch_generate(m, cond, u, steps):
    """The sampling loop, one step at a time, in torch operators: ``cond [n, T, L 2R]``, ``u [n, T]`` -> codes ``[n, steps]``."""
    R, L, A = m.n_residual_channels, m.n_layers, m.n_out_channels
    n = cond.shape[0]
    W0 = [c.conv.weight[:, :, 0].t().contiguous() for c in m.dilate_layers]
    W1 = [c.conv.weight[:, :, 1].t().contiguous() for c in m.dilate_layers]
    Ws = [c.conv.weight[:, :, 0].t().contiguous() for c in m.skip_layers]
    Wr = [c.conv.weight[:, :, 0].t().contiguous() for c in m.res_layers]
    Wo, We = m.conv_out.conv.weight[:, :, 0].t().contiguous(), m.conv_end.conv.weight[:, :, 0].t().contiguous()
    hist = [[] for _ in range(L)]
    zero = torch.zeros((n, R), device=cond.device)
    y = torch.full((n,), A // 2, dtype=torch.long, device=cond.device)
    out = []
    with torch.no_grad():
        for t in range(steps):
            x = m.embed.weight[y]
            skip = 0
            for l, d in enumerate(m.dilations):
                xd = hist[l][t - d] if t >= d else zero
                hist[l].append(x)
                z = xd @ W0[l] + x @ W1[l] + m.dilate_layers[l].conv.bias + cond[:, t, l * 2 * R:(l + 1) * 2 * R]
                acts = torch.tanh(z[:, :R]) * torch.sigmoid(z[:, R:])
                skip = skip + acts @ Ws[l] + m.skip_layers[l].conv.bias
                if l < L - 1:
                    x = x + acts @ Wr[l] + m.res_layers[l].conv.bias
            logits = torch.relu(torch.relu(skip) @ Wo) @ We
            c = torch.cumsum(torch.exp(logits - logits.max(-1, keepdim=True).values), -1)
            y = (c >= u[:, t:t + 1] * c[:, -1:]).float().argmax(-1)
            out.append(y)
    return torch.stack(out, 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--window', type=float, default=0.5, help='least device time of a training window, seconds')
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--steps', type=int, default=2048, help='time steps of a sampling measurement')
    ap.add_argument('--torch-steps', type=int, default=300)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_wavenet.py needs an MI355X'
    import padertorch_amd as pt
    from padertorch_amd.ops import wavenet as wn
    dev = torch.device('cuda:0')
    torch.manual_seed(22)
    m = pt.modules.WaveNet(**NET).to(dev)
    lines = []

    def emit(res):
        print(json.dumps(res), flush=True)
        lines.append(json.dumps(res))

    # ------------------------------------------------------------------ training step
    B, T, Tf = 4, 16000, 66
    features = torch.randn(B, NET['n_cond_channels'], Tf, device=dev)
    audio = torch.rand(B, T, device=dev) * 2 - 1
    w = torch.randn(B, NET['n_out_channels'], T, device=dev)
    params = list(m.parameters())

    def ours():
        return torch.autograd.grad((m(features, audio)[0] * w).sum(), params)

    def theirs():
        return torch.autograd.grad((torch_forward(m, features, audio) * w).sum(), params)

    with torch.no_grad():
        a, b = m(features, audio)[0], torch_forward(m, features, audio)
    res = dict(what='training step (forward + backward)', B=B, T=T, net=NET,
               max_rel_difference_output=float(f'{float((a - b).abs().max() / b.abs().max()):.3g}'))
    # accuracy at this size: both against the fp64 restatement (tests/wavenet_ref.py) on the GPU, worst parameter gradient of each
    import wavenet_ref as ref
    p64 = {k: v.detach().double().requires_grad_() for k, v in m.state_dict().items()}
    want = ref.forward(p64, features.double(), audio.double(), NET['upsamp_window'], NET['upsamp_stride'], NET['fading'], NET['max_dilation'])[0]
    g64 = torch.autograd.grad((want * w.double()).sum(), list(p64.values()))
    names = list(p64)
    for label, out, grads in (('hip', a, ours()), ('torch_conv1d', b, theirs())):
        devs = {k: float((x - y).abs().max() / y.abs().max()) for k, x, y in zip(names, grads, g64)}
        worst = max(devs, key=devs.get)
        res[label + '_vs_fp64'] = dict(output=float(f'{float((out.detach() - want.detach()).abs().max() / want.detach().abs().max()):.3g}'),
                                       worst_gradient=float(f'{devs[worst]:.3g}'), worst_gradient_of=worst,
                                       gradients={k: float(f'{v:.2g}') for k, v in devs.items() if not k.startswith(('dilate', 'res_', 'skip'))},
                                       worst_layer_gradient=float(f'{max(v for k, v in devs.items() if k.startswith(("dilate", "res_", "skip"))):.3g}'))
    del a, b, want, g64, p64, grads
    runs = {'hip': ours, 'torch_conv1d': theirs}
    reps, times = {}, {k: [] for k in runs}
    for name, fn in runs.items():
        timed(fn, 2)
        reps[name] = max(2, int(1.1 * args.window / timed(fn, 3)) + 1)
    for _ in range(args.rounds):
        for name, fn in runs.items():
            times[name].append(timed(fn, reps[name]))
    for name, t in times.items():
        res[name] = dict(median_ms=round(statistics.median(t) * 1e3, 3), min_ms=round(min(t) * 1e3, 3), max_ms=round(max(t) * 1e3, 3),
                         steps_per_window=reps[name])
    res['torch_over_hip'] = round(res['torch_conv1d']['median_ms'] / res['hip']['median_ms'], 2)
    emit(res)

    # ------------------------------------------------------------------ sampling
    steps = args.steps
    Tf_s = -(-(steps + 512) // 256) + 1
    packed = m.packed_weights()
    for nseq in (1, 4, 16):
        with torch.no_grad():
            cond = m._cond(torch.randn(nseq, NET['n_cond_channels'], Tf_s, device=dev))[:, :steps].contiguous()
        u = torch.rand(nseq, steps, device=dev)

        def run(spl):
            return wn.generate(packed, m.embed.weight.detach(), cond, u, m.dilations, NET['n_skip_channels'], NET['n_out_channels'],
                               steps_per_launch=spl)[0]
        run(steps)
        t = [timed(lambda: run(steps), 1) for _ in range(args.rounds)]
        med = statistics.median(t)
        ts = min(args.torch_steps, steps)
        torch_generate(m, cond, u, 20)
        t_torch = timed(lambda: torch_generate(m, cond, u, ts), 1)
        same = bool(torch.equal(run(steps)[:, :ts], torch_generate(m, cond, u, ts)))
        res = dict(what='sampling', sequences=nseq, steps=steps, workgroups=-(-nseq // 4),
                   hip=dict(median_s=round(med, 4), min_s=round(min(t), 4), max_s=round(max(t), 4), us_per_step=round(med / steps * 1e6, 2),
                            samples_per_s=round(nseq * steps / med, 1), steps_for_100ms=int(0.1 / (med / steps))),
                   torch_loop=dict(steps=ts, seconds=round(t_torch, 4), us_per_step=round(t_torch / ts * 1e6, 2),
                                   samples_per_s=round(nseq * ts / t_torch, 1)),
                   codes_equal_torch_loop=same)
        res['torch_over_hip_per_step'] = round(res['torch_loop']['us_per_step'] / res['hip']['us_per_step'], 2)
        emit(res)
    emit(dict(what='default', STEPS_PER_LAUNCH=wn.STEPS_PER_LAUNCH))
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
