"""``contrib.mk.modules.transformer`` on the GPU against the record of the reference's own classes run in fp64 on the CPU
(``tests/golden/g31_mk_transformer*.npz``, ``make_golden_mk_transformer.py``): strict ``state_dict`` load, output and every gradient.

Gates: per quantity four times the reference's own fp32-vs-fp64 difference (stored by the generator) plus the fp32 spacing 2^-23,
relative to the quantity's largest fp64 magnitude.  The norms are compared against torch's functions in fp64 on the CPU, gated the same
way with torch's own fp32 CPU run in the reference's place.  Every test appends its worst ratio to ``profiles/mk_transformer_gates.txt``."""
import importlib.util
from pathlib import Path

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

HERE = Path(__file__).resolve().parent
_spec = importlib.util.spec_from_file_location('make_golden_mk_transformer', HERE / 'golden' / 'make_golden_mk_transformer.py')
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)
GOLDEN = {**np.load(HERE / 'golden' / 'g31_mk_transformer.npz'), **np.load(HERE / 'golden' / 'g31_mk_transformer_wide.npz')}
GATES = HERE.parent / 'profiles' / 'mk_transformer_gates.txt'


def tf():
    from padertorch_amd.contrib.mk.modules import transformer
    return transformer


def check(label, got, want, top, d32):
    """``got``, ``want``: name -> array; ``top``, ``d32``: name -> the quantity's magnitude and the reference's own fp32 error."""
    assert sorted(got) == sorted(want), (sorted(got), sorted(want))
    ratios = {}
    for k in want:
        err = float(np.abs(got[k].detach().cpu().double().numpy() - want[k]).max()) / float(top[k])
        ratios[k] = (err / (4 * float(d32[k]) + 2. ** -23), err)
    worst = max(ratios, key=lambda k: ratios[k][0])
    line = f'{label:40s} {len(want):3d} quantities, worst {ratios[worst][0]:.3g} of its gate: {worst} (error {ratios[worst][1]:.3g})'
    print(line, {k: f'{v[1]:.3g}' for k, v in ratios.items()})
    GATES.parent.mkdir(exist_ok=True)
    with open(GATES, 'a') as f:
        f.write(line + ('' if ratios[worst][0] <= 1 else '   FAILED') + '\n')
    assert ratios[worst][0] <= 1, (label, {k: v for k, v in ratios.items() if v[0] > 1})


def against_record(case, module, fn, ins):
    prefix = f'{case}/p_'
    module.load_state_dict({k[len(prefix):]: torch.from_numpy(GOLDEN[k]) for k in GOLDEN if k.startswith(prefix)}, strict=True)
    module.cuda()
    leaves = {k: torch.from_numpy(v).cuda().requires_grad_() for k, v in ins.items() if k != 'w'}
    y = fn(module, leaves)
    named = list(leaves.items()) + list(module.named_parameters())
    grads = torch.autograd.grad((y * torch.from_numpy(ins['w']).cuda()).sum(), [t for _, t in named])
    got = {'y': y, **{f'g_{n}': g for (n, _), g in zip(named, grads)}}
    check(case, got, *({k: GOLDEN[f'{case}/{p}{k}'] for k in got} for p in ('', 'top_', 'd32_')))


@pytest.mark.parametrize('case', sorted(gen.MHA))
def test_multihead_attention(case):
    cfg = gen.MHA[case]
    ins, mask = gen.mha_inputs(case)
    if cfg.get('causal'):
        kpm = None
    elif cfg.get('float_mask'):
        kpm = torch.from_numpy(mask).cuda()
    else:
        kpm = torch.tensor(cfg['klen'], dtype=torch.int32, device='cuda')

    def fn(m, leaves):
        key, value = leaves.get('key', leaves['query']), leaves.get('value', leaves['query'])
        y, weights = m(leaves['query'], key, value, key_padding_mask=kpm, is_causal=cfg.get('causal', False))
        assert weights is None
        return y
    against_record(case, gen.build_mha(tf().MultiheadAttention, case), fn, ins)


@pytest.mark.parametrize('case', sorted(gen.ROPE))
def test_rope_alone(case):
    against_record(case, tf().RoPE(gen.ROPE[case][-1]), lambda m, leaves: m(leaves['x']), gen.rope_inputs(case))


@pytest.mark.parametrize('case', sorted(gen.ENCODERS))
def test_transformer_encoder(case):
    """Two layers, ``norm='dyt'``, attention with ``rope + rms_norm``, the encoder's ``output_norm='layer'``, lengths ``[70, 33, 5]``.
    The second layer's attention is diffuse and its query / key gradients are small differences ``dp - delta`` of large terms: the case
    that needs the backward's row term formed from the recomputed probabilities (``attn_delta_bias_kernel``)."""
    against_record(case, gen.build_encoder(tf(), case), lambda m, leaves: m(leaves['x'], list(gen.ENC_LENGTHS))[0], gen.encoder_inputs())


def torch_norm(kind, dtype, res, t):
    """torch's own functions on the CPU: ``s = x (+ r)``, ``y = norm(s)``; values and the gradients of ``sum(y gy) (+ sum(s gs))``."""
    t = {k: v.to(dtype).requires_grad_() for k, v in t.items()}
    N = t['x'].shape[-1]
    s = t['x'] + t['r'] if res else t['x']
    if kind == 'layer':
        y, params = F.layer_norm(s, (N,), t['weight'], t['bias'], 1e-5), ['weight', 'bias']
    elif kind == 'rms':
        y, params = F.rms_norm(s, (N,), t['weight'], float(torch.finfo(torch.float32).eps)), ['weight']
    else:
        y, params = torch.tanh(t['alpha'] * s) * t['weight'] + t['bias'], ['weight', 'bias', 'alpha']
    names = ['x'] + (['r'] if res else []) + params
    loss = (y * t['gy']).sum() + ((s * t['gs']).sum() if res else 0.)
    grads = torch.autograd.grad(loss, [t[n] for n in names])
    return {'y': y.detach(), **({'s': s.detach()} if res else {}), **{f'g_{n}': g for n, g in zip(names, grads)}}, params


@pytest.mark.parametrize('N', [24, 70])                      # 70: not a multiple of the 64 lanes that stride a row
@pytest.mark.parametrize('res', [False, True])
@pytest.mark.parametrize('kind', ['layer', 'rms', 'dyt'])
def test_row_norm(kind, res, N):
    from padertorch_amd.ops.mk_attention import row_norm
    gen_ = torch.Generator().manual_seed(41)
    t = {k: torch.randn(3, 37, N, generator=gen_) for k in ('x', 'r', 'gy', 'gs')}
    t.update(weight=1 + 0.3 * torch.randn(N, generator=gen_), bias=0.3 * torch.randn(N, generator=gen_), alpha=torch.tensor([0.7]))
    want, params = torch_norm(kind, torch.float64, res, t)
    own, _ = torch_norm(kind, torch.float32, res, t)
    top = {k: v.abs().max() for k, v in want.items()}
    d32 = {k: float((own[k].double() - want[k]).abs().max() / top[k]) for k in want}
    g = {k: v.cuda().requires_grad_() for k, v in t.items()}
    out = row_norm(kind, g['x'], g['r'] if res else None, **{k: g[k] for k in params})
    s, y = out if res else (None, out)
    names = ['x'] + (['r'] if res else []) + params
    grads = torch.autograd.grad((y * g['gy']).sum() + ((s * g['gs']).sum() if res else 0.), [g[n] for n in names])
    got = {'y': y, **({'s': s} if res else {}), **{f'g_{n}': v for n, v in zip(names, grads)}}
    check(f'row_norm {kind} res={res} N={N}', got, {k: v.numpy() for k, v in want.items()}, top, d32)
