#!/usr/bin/env python3
"""Generate tests/golden/g14_convnet.npz by importing the REAL reference's ConvNet (padertorch/modules/convnet.py).

Run in the build container only (needs /root/reference):

    python tests/golden/make_golden_convnet.py

The reference is imported exactly as make_golden_tas_coders.py does.  The output is data only.  Four configurations
(input_size, hidden_channels, kernel_size, num_blocks, num_repeats, norm, B, T):

    8/16/3/3x2/gLN/3/37   baseline
    8/16/3/2x1/cLN/2/37   cLN
    5/7/4/2x1/gLN/2/9     even kernel (asymmetric pad), odd channel counts, dilation 2 against T = 9
    8/16/3/5x1/gLN/1/9    dilations 8 and 16 exceed T: every off-centre tap lies in the padding; B = 1

The input ``x [B, T, N]`` and the functional's weights ``r`` are NOT stored: ``inputs(case, seed)`` draws them from a seeded numpy
RandomState and the tests call the same function.  The norms' gamma are drawn from [0.5, 1.5], their beta from [-0.5, 0.5], the PReLU
slopes from [0.1, 0.4] (at their initial 1 / 0 / 0.25 they would hide errors).

PReLU ties: a pre-activation whose sign differs between an fp32 and the fp64 run changes an element-wise gradient by far more than any
gate, so per case the seed is moved until no PReLU input of the fp64 run lies within 1e-5 max|input| of zero (max over that PReLU's
input tensor); the margin reached (min |input| / max |input| over all PReLUs) is stored as ``c<i>_margin``, the seed as ``c<i>_seed``.

Keys per case ``c<i>_``: ``keys`` (json list: the state_dict keys in order), ``p_<key>`` every state_dict entry, ``y64`` / ``y32`` the
output of the fp64 / fp32 run, ``g64_x`` / ``g32_x`` and ``g64_<name>`` / ``g32_<name>`` the gradients of ``sum(y * r)`` w.r.t. the input and
every entry of ``named_parameters()`` (``names``: json list).
"""
import json
import sys
from pathlib import Path

HERE = Path(__file__).resolve().parent
REPO = HERE.parent.parent

import numpy as np  # noqa: E402

#: (input_size, hidden_channels, kernel_size, num_blocks, num_repeats, norm, B, T)
CASES = [(8, 16, 3, 3, 2, 'gLN', 3, 37), (8, 16, 3, 2, 1, 'cLN', 2, 37), (5, 7, 4, 2, 1, 'gLN', 2, 9), (8, 16, 3, 5, 1, 'gLN', 1, 9)]
TIE_MARGIN = 1e-5


def inputs(case, seed):
    """The seeded input ``x [B, T, N]`` and the weights ``r [B, T, N]`` of the functional ``sum(y * r)``."""
    N, _, _, _, _, _, B, T = case
    rng = np.random.RandomState(seed)
    return rng.randn(B, T, N).astype(np.float32), rng.randn(B, T, N).astype(np.float32)


def build(case, seed):
    import torch
    from padertorch.modules.convnet import ConvNet  # the reference
    N, H, K, blocks, repeats, norm, _, _ = case
    torch.manual_seed(seed)
    net = ConvNet(input_size=N, num_blocks=blocks, num_repeats=repeats, hidden_channels=H, kernel_size=K, norm=norm)
    rng = np.random.RandomState(seed + 1)
    with torch.no_grad():
        for name, p in net.named_parameters():
            leaf = name.rsplit('.', 1)[1]
            if 'activation_fn' in name:
                lo, hi = 0.1, 0.4
            elif '.conv.' not in name and 'norm' in name and leaf in ('gamma', 'weight'):
                lo, hi = 0.5, 1.5
            elif '.conv.' not in name and 'norm' in name and leaf in ('beta', 'bias'):
                lo, hi = -0.5, 0.5
            else:
                continue
            p.copy_(torch.from_numpy(rng.uniform(lo, hi, size=tuple(p.shape)).astype(np.float32)))
    return net


def run(net, case, seed, dtype, margins=None):
    import torch
    x0, r0 = inputs(case, seed)
    net = net.to(dtype)
    for p in net.parameters():
        p.grad = None
    hooks = []
    if margins is not None:
        for m in net.modules():
            if isinstance(m, torch.nn.PReLU):
                hooks.append(m.register_forward_hook(
                    lambda _m, args, _out: margins.append(float(args[0].detach().abs().min() / args[0].detach().abs().max()))))
    x = torch.from_numpy(x0).to(dtype).requires_grad_()
    y = net(x, None)
    (y * torch.from_numpy(r0).to(dtype)).sum().backward()
    for h in hooks:
        h.remove()
    grads = {name: p.grad.numpy().copy() for name, p in net.named_parameters()}
    return y.detach().numpy().copy(), x.grad.numpy().copy(), grads


def main():
    sys.path[:0] = [str(HERE / 'ref_shim'), str(REPO), '/root/reference']
    import torch

    torch.set_num_threads(1)
    torch.use_deterministic_algorithms(True)
    out = {}
    for i, case in enumerate(CASES):
        seed = 1400 + 100 * i
        while True:
            net = build(case, seed)
            params = {k: v.numpy().copy() for k, v in net.state_dict().items()}
            margins = []
            y64, gx64, g64 = run(net, case, seed, torch.float64, margins)
            if min(margins) >= TIE_MARGIN:
                break
            seed += 1
        y32, gx32, g32 = run(net, case, seed, torch.float32)
        p = f'c{i}_'
        out[p + 'seed'], out[p + 'margin'] = np.array(seed), np.array(min(margins))
        out[p + 'keys'] = np.array(json.dumps(list(params)))
        out[p + 'names'] = np.array(json.dumps(list(g64)))
        for k, v in params.items():
            out[p + 'p_' + k] = v
        out[p + 'y64'], out[p + 'y32'], out[p + 'g64_x'], out[p + 'g32_x'] = y64, y32, gx64, gx32
        for k in g64:
            out[p + 'g64_' + k], out[p + 'g32_' + k] = g64[k], g32[k]
        worst = max(float(np.abs(g32[k] - g64[k]).max() / np.abs(g64[k]).max()) for k in g64)
        print(case, 'seed', seed, 'margin %.2e' % min(margins), 'fp32 vs fp64: y %.1e dx %.1e worst parameter gradient %.1e' % (
            np.abs(y32 - y64).max() / np.abs(y64).max(), np.abs(gx32 - gx64).max() / np.abs(gx64).max(), worst))
    out['cases'] = np.array(json.dumps(CASES))
    path = HERE / 'g14_convnet.npz'
    np.savez_compressed(path, **out)
    print(path, path.stat().st_size, 'bytes')


if __name__ == '__main__':
    main()
