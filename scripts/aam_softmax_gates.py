"""The gates of tests/test_gpu_aam_softmax.py: that file's restatement of the angular-margin softmax (and torch's batch norm) in fp32 on
the CPU against its fp64 run over the test's own cases; per quantity the largest error relative to the largest magnitude of the quantity
in the case, and four times it (two legitimate fp32 evaluations with different summation orders).  No GPU needed.

    python scripts/aam_softmax_gates.py >> profiles/aam_softmax_gates.txt
"""
import sys
from pathlib import Path

import torch
import torch.nn.functional as F

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from padertorch_amd.ops.aam_softmax import DEFAULTS  # noqa: E402
from tests.test_gpu_aam_softmax import BN_GATES, GATES, SHAPES, inputs, rel, restatement  # noqa: E402

worst = dict.fromkeys(GATES, 0.)
for loss_type in ('aam', 'arcface', 'sphereface'):
    for shape in SHAPES:
        for reduce in ('mean', None):
            e, w, y, gout = inputs(*shape)
            want = restatement(e, w, y, loss_type, *DEFAULTS[loss_type], gout=None if reduce == 'mean' else gout)
            got = restatement(e.float(), w.float(), y, loss_type, *DEFAULTS[loss_type], gout=None if reduce == 'mean' else gout.float())
            for k, a, b in zip(GATES, got, want):
                worst[k] = max(worst[k], rel(a, b))
bn = dict.fromkeys(BN_GATES, 0.)
for B, E in ((2, 3), (37, 70)):
    for training in (True, False):
        g = torch.Generator().manual_seed(B)
        x = torch.randn(B, E, generator=g, dtype=torch.float64) * 3 + 1
        gy = torch.randn(B, E, generator=g, dtype=torch.float64)
        rm, rv = torch.randn(E, generator=g, dtype=torch.float64), torch.rand(E, generator=g, dtype=torch.float64) + 0.5
        out = []
        for dt in (torch.float32, torch.float64):
            xs, m, v = x.to(dt).requires_grad_(True), rm.to(dt), rv.to(dt)
            ys = F.batch_norm(xs, m, v, training=training, momentum=0.1, eps=1e-5)
            ys.backward(gy.to(dt))
            out.append((ys.detach(), xs.grad, m, v))
        for k, a, b in zip(BN_GATES, *out):
            bn[k] = max(bn[k], rel(a, b))
print('quantity        fp32 restatement vs fp64    gate (x 4)')
for k, v in {**worst, **{'bn ' + k: v for k, v in bn.items()}}.items():
    print(f'{k:<16}{v:<28.3e}{4 * v:.1e}')
