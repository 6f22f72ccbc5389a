#!/usr/bin/env python3
"""Generate tests/golden/g31_mk_transformer.npz from the REAL reference's ``padertorch/contrib/mk/modules/transformer.py`` on the CPU.

    python tests/golden/make_golden_mk_transformer.py <path of a padertorch checkout>

The reference is imported as make_golden_cpc.py imports it (the repository root and ``ref_shim`` on the path).  The output is data only.

``MHA`` lists the ``MultiheadAttention`` cases, ``ROPE`` the stand-alone ``RoPE`` shapes, ``ENCODERS`` the ``TransformerEncoder`` run
(pre-norm; post-norm cannot be recorded, the reference's layer raises a ``TypeError`` there).  The reference's
``MultiheadAttention.forward`` casts to fp32 (:762), so the fp64 record goes through ``forward64`` below, which CALLS the reference's own
``prepare_attention``, ``F.normalize``, ``attention_fn`` and ``out_proj``; in fp32 it is asserted to equal ``forward`` bit for bit.  For the fp64 run the RMS modules' ``eps`` is set to the fp32 epsilon, so that both precisions
compute one function, and ALL parameters are randomised after construction (``reset_parameters`` leaves the RMS weights at 0).

The inputs are not stored: the test takes them from ``mha_inputs`` / ``rope_inputs`` / ``encoder_inputs`` below (fp32, the functional's
weight ``w`` among them).  Keys, per case ``<c>``: ``<c>/p_<state_dict key>`` (buffers included), ``<c>/y`` (fp64), ``<c>/g_<name>`` (fp64
gradients of ``sum(y w)`` in the inputs and parameters), ``<c>/d32_<quantity>`` = the reference's own fp32-vs-fp64 difference relative to ``<c>/top_<quantity>``, the quantity's largest fp64 magnitude.  A gradient that is
analytically zero (``lin_key.bias`` where nothing but the softmax follows the key projection: fp64 magnitude below 1e-9 of its weight's)
is measured against its module's weight gradient instead.  The test gates at ``4 d32 + 2^-23``.
"""
import inspect
import json
import sys
from pathlib import Path

import numpy as np

HERE = Path(__file__).resolve().parent
REPO = HERE.parent.parent
RMS_EPS = float(np.finfo(np.float32).eps)
#: ``signatures`` (json): the constructor parameter names of these classes of the reference
CLASSES = ['Linear', 'PositionalEncoding', 'RoPE', 'DynamicTanh', 'LayerNorm', 'ScaledDotProductAttention', 'MultiheadAttention',
           'TransformerNormBlock', 'EncoderLayer', 'TransformerEncoderLayer', 'TransformerEncoder']

SELF, CROSS = dict(Tq=70, Tk=70, klen=[70, 33, 5]), dict(Tq=70, Tk=45, klen=[45, 33, 5], kdim=10, vdim=14)
FULL = dict(rope=True, rms_norm=True, linear_attention_bias=True)
MHA = {
    'self_rope': dict(SELF, opts=dict(rope=True)),
    'self_full': dict(SELF, opts=FULL),
    'self_l2': dict(SELF, opts=dict(l2_normalization=True)),
    'self_lab': dict(SELF, opts=dict(linear_attention_bias=True)),
    'causal_full': dict(SELF, opts=FULL, causal=True),
    'cross_rope': dict(CROSS, opts=dict(rope=True)),
    'cross_full': dict(CROSS, opts=FULL),
    'cross_l2_mask': dict(CROSS, opts=dict(l2_normalization=True), float_mask=True),
    'wide_full': dict(SELF, opts=FULL, embed_dim=80),
}
ROPE = {'rope3': (3, 70, 12), 'rope4': (2, 2, 33, 40)}
ENCODERS = {'enc_pre': True}                 # pre_norm=False: the reference's layer raises (F.softplus of the int layer_scale, :970)
ENC_LENGTHS = [70, 33, 5]
B = 3
SECOND_FILE = ('wide_', 'enc_', 'rope')      # the cases of g31_mk_transformer_wide.npz (one file would pass the size limit of the repository)


def randomise(module, seed):
    import torch
    gen = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for p in module.parameters():
            p.copy_(torch.randn(p.shape, generator=gen) * (0.3 if p.ndim > 1 else 0.2) + (1. if p.ndim == 1 and p.numel() > 1 else 0.))
    return module


def build_mha(cls, case):
    cfg = MHA[case]
    return randomise(cls(cfg.get('embed_dim', 24), 2, kdim=cfg.get('kdim'), vdim=cfg.get('vdim'), **cfg['opts']), 3100 + sorted(MHA).index(case))


def build_encoder(tf, case):
    attn = tf.MultiheadAttention(24, 2, rope=True, rms_norm=True)
    layer = tf.TransformerEncoderLayer(24, attn, 'relu', nhead=2, dim_feedforward=48, norm='dyt', pre_norm=ENCODERS[case])
    net = tf.TransformerEncoder(16, layer, num_layers=2, output_norm='layer', positional_encoding=tf.PositionalEncoding(24, max_len=100),
                                use_activation_checkpointing=False)
    return randomise(net, 3200 + sorted(ENCODERS).index(case))


def mha_inputs(case):
    cfg = MHA[case]
    rng = np.random.RandomState(310 + sorted(MHA).index(case))
    E = cfg.get('embed_dim', 24)
    query = rng.randn(B, cfg['Tq'], E).astype(np.float32)
    ins = dict(query=query, w=rng.randn(B, cfg['Tq'], E).astype(np.float32))
    if 'kdim' in cfg:
        ins['key'] = rng.randn(B, cfg['Tk'], cfg['kdim']).astype(np.float32)
        ins['value'] = rng.randn(B, cfg['Tk'], cfg['vdim']).astype(np.float32)
    mask = np.where(np.arange(cfg['Tk'])[None] < np.array(cfg['klen'])[:, None], 0., -np.inf).astype(np.float32)
    return ins, mask


def rope_inputs(case):
    rng = np.random.RandomState(320 + len(ROPE[case]))
    return dict(x=rng.randn(*ROPE[case]).astype(np.float32), w=rng.randn(*ROPE[case]).astype(np.float32))


def encoder_inputs():
    rng = np.random.RandomState(330)
    return dict(x=rng.randn(B, 70, 16).astype(np.float32), w=rng.randn(B, 70, 24).astype(np.float32))


def forward64(self, query, key, value, key_padding_mask=None, is_causal=False):
    """``MultiheadAttention.forward`` without the cast to fp32 (:762): the reference's own methods, called in its order."""
    import torch.nn.functional as F
    B_, Tq, _ = query.shape
    q, k, v, key_padding_mask = self.prepare_attention(query, key, value, key_padding_mask)
    if self.l2_normalization:
        q = F.normalize(q, p=2, dim=-1)
        k = F.normalize(k, p=2, dim=-1)
    x, attn_weights = self.attention_fn(q, k, v, attn_mask=key_padding_mask, is_causal=is_causal)
    x = x.transpose(1, 2).contiguous().view(B_, Tq, self.embed_dim)
    return self.dropout(self.out_proj(x)), attn_weights


def set_rms_eps(module):
    import torch
    for m in module.modules():
        if isinstance(m, torch.nn.RMSNorm):
            m.eps = RMS_EPS


def run(fn, module, ins, dtype):
    """``y = fn(leaves)``; gradients of ``sum(y w)`` in the float inputs and the parameters."""
    import torch
    module = module.to(dtype)
    leaves = {k: torch.from_numpy(v).to(dtype).requires_grad_() for k, v in ins.items() if k != 'w'}
    y = fn(module, leaves)
    named = list(leaves.items()) + list(module.named_parameters())
    grads = torch.autograd.grad((y * torch.from_numpy(ins['w']).to(dtype)).sum(), [t for _, t in named])
    out = {'y': y.detach().double().numpy()}
    out.update({f'g_{n}': g.double().numpy() for (n, _), g in zip(named, grads)})
    return out


def scales(r64):
    """The magnitude every quantity is measured against (see the module docstring for the analytically zero gradients)."""
    top = {k: float(np.abs(v).max()) for k, v in r64.items()}
    for k in list(top):
        if k.endswith('.bias') and k[:-4] + 'weight' in top and top[k] < 1e-9 * top[k[:-4] + 'weight']:
            top[k] = top[k[:-4] + 'weight']
    return top


def record(out, case, module, fn, ins):
    import copy
    import torch
    state = {k: v.detach().clone() for k, v in module.state_dict().items()}
    r32 = run(fn, copy.deepcopy(module), ins, torch.float32)
    m64 = copy.deepcopy(module)
    set_rms_eps(m64)
    r64 = run(fn, m64, ins, torch.float64)
    top = scales(r64)
    for k, v in state.items():
        out[f'{case}/p_{k}'] = v.numpy()
    worst = 0.
    for k, v in r64.items():
        assert np.isfinite(v).all() and np.isfinite(r32[k]).all(), (case, k)
        out[f'{case}/{k}'] = v
        out[f'{case}/top_{k}'] = np.array(top[k])
        out[f'{case}/d32_{k}'] = np.array(np.abs(r32[k] - v).max() / top[k])
        worst = max(worst, float(out[f'{case}/d32_{k}']))
    print(f'{case:16s} {len(r64):3d} quantities, fp32 vs fp64: y {float(out[f"{case}/d32_y"]):.3g}, worst {worst:.3g}')


def main():
    sys.path[:0] = [str(HERE / 'ref_shim'), str(REPO), sys.argv[1]]
    import torch
    from padertorch.contrib.mk.modules import transformer as tf
    out = {'signatures': json.dumps({n: list(inspect.signature(getattr(tf, n).__init__).parameters)[1:] for n in CLASSES})}
    for case, cfg in MHA.items():
        module = build_mha(tf.MultiheadAttention, case)
        ins, mask = mha_inputs(case)
        causal = cfg.get('causal', False)

        def call(forward):
            def fn(m, leaves):
                key, value = leaves.get('key', leaves['query']), leaves.get('value', leaves['query'])
                kpm = None if causal else torch.from_numpy(mask).to(leaves['query'].dtype)
                return forward(m, leaves['query'], key, value, key_padding_mask=kpm, is_causal=causal)[0]
            return fn
        with torch.no_grad():
            leaves = {k: torch.from_numpy(v) for k, v in ins.items()}
            assert torch.equal(call(forward64)(module, leaves), call(tf.MultiheadAttention.forward)(module, leaves)), case
        record(out, case, module, call(forward64), ins)
    for case, shape in ROPE.items():
        record(out, case, tf.RoPE(shape[-1]), lambda m, leaves: m(leaves['x']), rope_inputs(case))
    tf.MultiheadAttention.forward = forward64
    for case in ENCODERS:
        record(out, case, build_encoder(tf, case), lambda m, leaves: m(leaves['x'], list(ENC_LENGTHS))[0], encoder_inputs())
    second = {k: v for k, v in out.items() if k.startswith(SECOND_FILE)}
    np.savez_compressed(HERE / 'g31_mk_transformer.npz', **{k: v for k, v in out.items() if k not in second})
    np.savez_compressed(HERE / 'g31_mk_transformer_wide.npz', **second)


if __name__ == '__main__':
    main()
