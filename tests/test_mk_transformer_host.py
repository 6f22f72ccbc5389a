"""``contrib.mk.modules.transformer`` without a GPU: the reference's constructor signatures and ``state_dict`` keys (from the record of
``make_golden_mk_transformer.py``), the options that are not ported, and the refusal of CPU tensors."""
import importlib.util
import inspect
import json
from pathlib import Path

import numpy as np
import pytest
import torch

HERE = Path(__file__).resolve().parent
_spec = importlib.util.spec_from_file_location('make_golden_mk_transformer', HERE / 'golden' / 'make_golden_mk_transformer.py')
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)
GOLDEN = {**np.load(HERE / 'golden' / 'g31_mk_transformer.npz'), **np.load(HERE / 'golden' / 'g31_mk_transformer_wide.npz')}


def tf():
    from padertorch_amd.contrib.mk.modules import transformer
    return transformer


def test_constructor_signatures_are_the_references():
    for name, params in json.loads(str(GOLDEN['signatures'])).items():
        assert list(inspect.signature(getattr(tf(), name).__init__).parameters)[1:] == params, name


@pytest.mark.parametrize('case', sorted(gen.MHA) + sorted(gen.ENCODERS))
def test_state_dict_keys_are_the_records(case):
    module = gen.build_mha(tf().MultiheadAttention, case) if case in gen.MHA else gen.build_encoder(tf(), case)
    prefix = f'{case}/p_'
    record = {k[len(prefix):]: tuple(GOLDEN[k].shape) for k in GOLDEN if k.startswith(prefix)}
    assert {k: tuple(v.shape) for k, v in module.state_dict().items()} == record


def layer(**kw):
    return tf().TransformerEncoderLayer(8, tf().MultiheadAttention(8, 2), 'relu', **kw)


@pytest.mark.parametrize('name, make', [
    ('magnitude_preserving', lambda: tf().MultiheadAttention(8, 2, magnitude_preserving=True)),
    ('magnitude_preserving', lambda: tf().Linear(4, 4, magnitude_preserving=True)),
    ('add_bias_kv', lambda: tf().MultiheadAttention(8, 2, add_bias_kv=True)),
    ('flash_attention', lambda: tf().MultiheadAttention(8, 2, flash_attention=True)),
    ('cond_dim', lambda: tf().DynamicTanh(8, cond_dim=4)),
    ('cond_dim', lambda: tf().LayerNorm(8, cond_dim=4)),
    ('cond_dim', lambda: layer(cond_dim=4)),
    ('normalize_skip_connections', lambda: layer(normalize_skip_connections=True)),
    ('pre_norm', lambda: layer(pre_norm=False)),
    ("norm='rms'", lambda: layer(norm='rms')),
    ('is_causal=True with Tq != Tk', lambda: tf().ScaledDotProductAttention()(*(torch.zeros(1, 2, t, 4) for t in (3, 5, 5)), is_causal=True)),
    ('odd head size', lambda: tf().MultiheadAttention(6, 2, rope=True)),
    ('MAX_HEAD', lambda: tf().MultiheadAttention(258, 2)),
])
def test_unported_options_raise_with_their_name(name, make):
    with pytest.raises(NotImplementedError, match=name):
        make()


def test_reset_parameters_zeroes_the_rms_weights_like_the_reference():
    mha = tf().MultiheadAttention(8, 2, rms_norm=True)
    total = {k: float(v.abs().sum()) for k, v in mha.state_dict().items()}
    assert total['q_norm.weight'] == 4.
    mha.reset_parameters(seed=1)
    total = {k: float(v.abs().sum()) for k, v in mha.state_dict().items()}
    assert total['q_norm.weight'] == 0. and total['k_norm.weight'] == 0. and total['lin_key.bias'] == 0. and total['lin_key.weight'] > 0.


def test_cpu_tensors_are_refused():
    from padertorch_amd.ops import mk_attention as mk
    x = torch.zeros(2, 5, 2, 4)
    for call in (lambda: mk.qk_prepare(x, x, theta=torch.ones(4)), lambda: mk.bias_attention(x, x, x, slopes=torch.ones(5)),
                 lambda: mk.row_norm('rms', x, x, torch.ones(4)), lambda: tf().RoPE(4)(x), lambda: tf().DynamicTanh(4)(x),
                 lambda: tf().MultiheadAttention(8, 2, rope=True)(x.view(2, 5, 8), x.view(2, 5, 8), x.view(2, 5, 8))):
        with pytest.raises(RuntimeError, match='no CPU fallback'):
            call()
