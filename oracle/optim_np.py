"""numpy restatement of the optimizer step: global-norm clip + Adam.  ORACLE - test infrastructure only.

Follows ``padertorch/train/optimizer.py``: ``Optimizer.clip_grad`` (``:31-42``, ``torch.nn.utils.clip_grad_norm_``:
``clip = min(1, max_norm / (norm + 1e-6))``) and ``Adam`` (``:79-90``, ``torch.optim.Adam`` without amsgrad: L2 weight decay
added to the gradient, ``lerp`` for ``exp_avg``, bias corrections taken in double on the host, ``denom = sqrt(v) /
sqrt(bc2) + eps``), as the header of ``csrc/optim.hip`` lists them.  ``tests/test_oracle_optim.py`` pins the float64 run
to torch's own float64 step.

The step computes in ``dtype`` (float64 unless asked otherwise): the float32 run of the same restatement is what the GPU
tests derive their gates from (``tests/test_gpu_optim_paths.py``).
"""
import math

import numpy as np


def clip_adam_step(p, g, m, v, t, *, lr, beta1, beta2, eps, weight_decay, max_norm=None, dtype=np.float64):
    """Step number ``t`` (1-based) on flat arrays: ``dict(p, m, v, norm, clip, terms)``.

    ``norm`` is the 2-norm of ``g`` and always taken in float64; in float32 it is rounded once and ``clip`` evaluated in
    float32 from there, so that a float32 run measures the element-wise arithmetic only (the norm has a gate of its own).
    ``terms[q]`` is, per element, the sum of the magnitudes that enter ``q``: what an error of ``q`` is measured in.
    """
    dtype = np.dtype(dtype).type
    p, g, m, v = (np.asarray(a, dtype) for a in (p, g, m, v))
    g64 = np.asarray(g, np.float64)
    norm = math.sqrt(float(np.square(g64).sum()))
    clip = dtype(1)
    if max_norm is not None:
        clip = min(dtype(1), dtype(max_norm) / (dtype(norm) + dtype(1e-6)))
    bc1 = 1.0 - float(beta1) ** t                       # double, whatever dtype is (torch: python floats)
    bc2 = 1.0 - float(beta2) ** t
    step_size, bc2_sqrt = dtype(lr / bc1), dtype(math.sqrt(bc2))
    b2, omb1, omb2, wd = dtype(beta2), dtype(1.0 - beta1), dtype(1.0 - beta2), dtype(weight_decay)

    gc = g * clip
    gg = gc + wd * p if weight_decay != 0 else gc
    m1 = m + omb1 * (gg - m)
    v1 = b2 * v + omb2 * gg * gg
    denom = np.sqrt(v1) / bc2_sqrt + dtype(eps)
    p1 = p - step_size * (m1 / denom)

    a = np.abs(gc) + wd * np.abs(p)
    terms = dict(m=np.abs(m) + omb1 * (np.abs(m) + a), v=b2 * v + omb2 * a * a, p=np.abs(p) + np.abs(p1 - p))
    return dict(p=p1, m=m1, v=v1, norm=norm, clip=clip, terms=terms)


def scaled_error(got, want, terms):
    """``max_i |got_i - want_i| / terms_i`` in float64 over every element; an element whose ``terms`` is 0 (nothing enters it) has to be
    exact: it counts 0 when it is and inf when it is not.  NaN anywhere gives inf."""
    got, want, terms = (np.asarray(a, np.float64).reshape(-1) for a in (got, want, terms))
    if got.size == 0:
        return 0.0
    num = np.abs(got - want)
    with np.errstate(divide='ignore', invalid='ignore'):
        r = np.where(terms > 0, num / terms, np.where(num == 0, 0.0, np.inf))
    r = np.where(np.isnan(r), np.inf, r)
    return float(r.max())
