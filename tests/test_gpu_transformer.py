"""The transformer stack on the GPU: the kernels of csrc/attention.hip and the modules on them against fp64 - the reference's golden run
(tests/golden/g24_transformer*.npz) or the restatement tests/transformer_ref.py on the same inputs.

Gates: the project's own, ``VALUE = 1e-5`` for values and ``GRAD = 2e-4`` for gradients, times ``max|want|``.  The reference's own fp32
run stays below a quarter of either on every layer-norm, norm=None, cross-attention and causal variant (asserted by the fixture's maker);
under norm='batch' its values do not (1.7e-6 and 1.9e-6 in the fixture, up to 6.2e-6 at other seeds), so there the gate of each quantity
is ``max(project gate, 4 x its recorded dev32)``.  A gradient that is analytically zero (every ``lin_key.bias``: softmax is shift
invariant; under norm='batch' with norm_first also the biases feeding a batch norm) has ``max|g64|`` ~1e-15: it is gated absolutely, at
``GRAD max|g64|`` of the same module's weight.  Every test appends its worst ratio to its gate to profiles/transformer_gates.txt."""
import math
from pathlib import Path

import pytest
import torch

import transformer_ref as ref

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
VALUE, GRAD = ref.VALUE, ref.GRAD
GATES = Path(__file__).resolve().parent.parent / 'profiles' / 'transformer_gates.txt'
TILE, KEY_TILE = 64, 32                  # ops.attention.TILE / KEY_TILE (asserted below)


class Worst:
    """The worst ratio-to-gate of one test; written to the gates file when the test leaves."""

    def __init__(self, label):
        self.label, self.ratio, self.what, self.n = label, 0., '-', 0

    def check(self, what, got, want, gate, scale=None):
        if scale is None:
            dev = ref.rel_dev(got, want)
        else:
            dev = float((torch.as_tensor(got).detach().cpu().double() - torch.as_tensor(want).double()).abs().max()) / scale
        self.n += 1
        if dev / gate >= self.ratio:
            self.ratio, self.what = dev / gate, f'{what} (deviation {dev:.3g}, gate {gate:.3g})'
        assert dev <= gate, (self.label, what, dev, gate)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        line = f'{self.label:60s} {self.n:4d} comparisons, worst {self.ratio:.3g} of its gate: {self.what}'
        print(line)
        GATES.parent.mkdir(exist_ok=True)
        with open(GATES, 'a') as f:
            f.write(line + ('' if exc[0] is None else '   FAILED') + '\n')
        return False


def att():
    from padertorch_amd.ops import attention
    return attention


def rand(*shape, seed, scale=1.0):
    return (torch.randn(*shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64) * scale).float()


def test_tile_constants():
    from padertorch_amd import _lib
    lib = _lib.load()
    assert (lib.ptmi_attn_tile(), lib.ptmi_attn_key_tile(), lib.ptmi_attn_max_head()) == (TILE, KEY_TILE, att().MAX_HEAD) == \
        (att().TILE, att().KEY_TILE, 128)


# ------------------------------------------------------------------------------------------------ 1. the attention op alone
def fp64_attention(q, k, v, seq_len, bidirectional, mask, w):
    """The restatement in fp64: ``(out, weights)`` with the reference's NaN rows, and the gradients of ``sum(out * w)`` over the rows
    that see a key (a row without one gives NaN gradients in the reference; the kernels give it none - ops/attention.py)."""
    q, k, v = (t.double().requires_grad_() for t in (q, k, v))
    out, weights = ref.scaled_dot_product_attention(q, k, v, seq_len, bidirectional, None if mask is None else mask.double())
    dead = torch.isnan(weights).any(-1)
    if dead.any():
        # the same rows with the dead ones given one visible key, then left out of the functional: finite gradients
        y = q @ k.transpose(-2, -1) / math.sqrt(k.shape[-1])
        if mask is not None:
            y = y + ref.log_mask(mask.double().expand(y.shape))
        y = y + (ref.log_mask(ref.get_causal_mask(y)) if not bidirectional else
                 (ref.log_mask(ref.length_mask(y, seq_len, 0, -1)) if seq_len is not None else 0))
        y = torch.where(dead[..., None], torch.zeros((), dtype=torch.float64), y)
        live = torch.softmax(y, -1) @ v
        (torch.where(dead[..., None], torch.zeros((), dtype=torch.float64), live) * w.double()).sum().backward()
    else:
        (out * w.double()).sum().backward()
    return out.detach(), weights.detach(), dead, (q.grad, k.grad, v.grad)


def gpu_attention(q, k, v, seq_len, bidirectional, mask, w, dead):
    q, k, v = (t.to(DEV).requires_grad_() for t in (q, k, v))
    out, weights = att().scaled_dot_product_attention(q, k, v, seq_len, bidirectional, None if mask is None else mask.to(DEV))
    assert not weights.requires_grad
    (torch.where(dead.to(DEV)[..., None], torch.zeros((), device=DEV), out) * w.to(DEV)).sum().backward()
    return out.detach(), weights, (q.grad, k.grad, v.grad)


SHAPES = [(1, 1), (TILE - 1, TILE - 1), (TILE, TILE), (TILE + 1, TILE + 1), (3 * TILE + 5, 3 * TILE + 5), (5, 9), (70, 11)]


@pytest.mark.parametrize('Tq, Tk', SHAPES)
@pytest.mark.parametrize('dh', [1, 8, 16, 40, 64, 128])
def test_attention_against_fp64(dh, Tq, Tk):
    B = 2
    with Worst(f'attention dh={dh} Tq={Tq} Tk={Tk}') as worst:
        for H in (1, 3):
            q, k, v = rand(B, H, Tq, dh, seed=1), rand(B, H, Tk, dh, seed=2), rand(B, H, Tk, dh, seed=3)
            w = rand(B, H, Tq, dh, seed=4)
            gen = torch.Generator().manual_seed(5)
            wide = (torch.rand(B, 1, Tq, Tk, generator=gen) > 0.3).float()
            row = (torch.rand(1, 1, 1, Tk, generator=gen) > 0.3).float()
            row[..., 0] = 1
            edge = [min(Tk, KEY_TILE + 1), min(Tk, TILE + 1)]           # one past a tile edge (of either tile size) where Tk allows
            cases = [('no mask', None, True, None), ('lengths [Tk, 1]', [Tk, 1], True, None), ('lengths past an edge', edge, True, None),
                     ('causal', None, False, None), ('mask [B, 1, Tq, Tk]', None, True, wide), ('mask [1, 1, 1, Tk]', None, True, row),
                     ('lengths + mask', [Tk, 1], True, wide), ('causal + mask', None, False, row)]
            for label, seq_len, bidirectional, mask in cases:
                label = f'H={H} {label}'
                want_out, want_w, dead, want_g = fp64_attention(q, k, v, seq_len, bidirectional, mask, w)
                out, weights, grads = gpu_attention(q, k, v, seq_len, bidirectional, mask, w, dead)
                worst.check(f'{label}: out', out, want_out, VALUE)
                worst.check(f'{label}: weights', weights, want_w, VALUE)
                live = ~dead
                if live.any():
                    sums = weights.cpu().double().sum(-1)[live]
                    assert float((sums - 1).abs().max()) <= 1e-6, (label, float((sums - 1).abs().max()))
                for name, a, b in zip(('dq', 'dk', 'dv'), grads, want_g):
                    if float(b.abs().max()) == 0.:              # (nothing visible but dead rows: exact zeros)
                        assert float(a.abs().max()) == 0., (label, name)
                    else:
                        worst.check(f'{label}: {name}', a, b, GRAD)
                if seq_len is not None and mask is None:
                    # the lengths as device data, int32 and int64: the same bits as the host list
                    for dtype in (torch.int32, torch.int64):
                        out2, w2 = att().scaled_dot_product_attention(q.to(DEV), k.to(DEV), v.to(DEV), torch.tensor(seq_len, dtype=dtype, device=DEV), True)
                        assert torch.equal(out2, out) and torch.equal(w2, weights), (label, dtype)


def test_causal_call_ignores_seq_len_and_v_may_be_wider():
    q, k, v = rand(2, 6, 4, seed=1).to(DEV), rand(2, 6, 4, seed=2).to(DEV), rand(2, 6, 8, seed=3).to(DEV)       # the reference's doctest shapes
    a, wa = att().scaled_dot_product_attention(q, k, v, seq_len=[6, 4], bidirectional=False)
    b, wb = att().scaled_dot_product_attention(q, k, v, bidirectional=False)
    assert torch.equal(a, b) and torch.equal(wa, wb) and a.shape == (2, 6, 8) and wa.shape == (2, 6, 6)
    with Worst('attention doctest shapes (dv = 8, d = 4)') as worst:
        want, want_w = ref.scaled_dot_product_attention(q.cpu().double(), k.cpu().double(), v.cpu().double(), [6, 4], True)
        got, got_w = att().scaled_dot_product_attention(q, k, v, seq_len=[6, 4], bidirectional=True)
        worst.check('out', got, want, VALUE)
        worst.check('weights', got_w, want_w, VALUE)
        zeros = torch.zeros(2, 6, 4, device=DEV)
        x, _ = att().scaled_dot_product_attention(zeros, k * 0, v, bidirectional=False)
        assert torch.equal(x[0, 0], v[0, 0])
        worst.check('uniform weights', x[0, -1], v[0].mean(0).cpu().double(), VALUE)


def test_row_without_a_visible_key_is_nan_and_its_neighbours_are_not():
    B, H, Tq, Tk, dh = 2, 3, TILE + 3, TILE + 7, 16
    q, k, v = rand(B, H, Tq, dh, seed=1).to(DEV), rand(B, H, Tk, dh, seed=2).to(DEV), rand(B, H, Tk, dh, seed=3).to(DEV)
    mask = torch.ones(B, 1, Tq, Tk, device=DEV)
    mask[0, 0, 5] = 0
    mask[1, 0, TILE] = 0
    out, weights = att().scaled_dot_product_attention(q, k, v, bidirectional=True, mask=mask)
    dead = torch.zeros(B, H, Tq, dtype=torch.bool, device=DEV)
    dead[0, :, 5] = dead[1, :, TILE] = True
    assert torch.equal(torch.isnan(out).all(-1), dead) and torch.equal(torch.isnan(out).any(-1), dead)
    assert torch.equal(torch.isnan(weights).all(-1), dead) and torch.equal(torch.isnan(weights).any(-1), dead)
    want, _ = ref.scaled_dot_product_attention(q.cpu().double(), k.cpu().double(), v.cpu().double(), None, True, mask.cpu().double())
    with Worst('attention with dead rows') as worst:
        worst.check('out', out, want, VALUE)
    # a length of zero: every row of that example
    out, weights = att().scaled_dot_product_attention(q, k, v, seq_len=[0, Tk], bidirectional=True)
    assert torch.isnan(out[0]).all() and torch.isnan(weights[0]).all() and not torch.isnan(out[1]).any() and not torch.isnan(weights[1]).any()


def test_need_weights_false_launches_no_weights_kernel(monkeypatch):
    from padertorch_amd import _lib
    q, k, v = rand(2, 3, 70, 16, seed=1).to(DEV), rand(2, 3, 70, 16, seed=2).to(DEV), rand(2, 3, 70, 16, seed=3).to(DEV)
    launched = []
    call = _lib.call

    def counting(symbol, *args, **kw):
        launched.append(symbol)
        return call(symbol, *args, **kw)
    monkeypatch.setattr(_lib, 'call', counting)
    out, weights = att().scaled_dot_product_attention(q, k, v, bidirectional=True, need_weights=False)
    assert weights is None and launched == ['ptmi_attn_forward']
    del launched[:]
    out2, weights = att().scaled_dot_product_attention(q, k, v, bidirectional=True)
    assert launched == ['ptmi_attn_forward', 'ptmi_attn_weights'] and weights.shape == (2, 3, 70, 70) and torch.equal(out, out2)
    # a stack never asks for them
    from padertorch_amd.contrib.je.modules import TransformerLayerStack
    net = TransformerLayerStack(10, 48, 40, 3, 2, bidirectional=True).to(DEV)
    del launched[:]
    y, _ = net(rand(2, 9, 10, seed=4).to(DEV), [9, 4])
    y.sum().backward()
    assert launched.count('ptmi_attn_forward') == 2 and launched.count('ptmi_attn_backward') == 2 and 'ptmi_attn_weights' not in launched
    # self-attention packs its input once for the three projections: two packing launches fewer per layer than without the sharing
    from padertorch_amd.contrib.je.modules import transformer as tf

    def packs():
        del launched[:]
        with torch.no_grad():
            out = net(rand(2, 9, 10, seed=4).to(DEV), [9, 4])[0]
        return launched.count('ptmi_pack_planes_n'), launched.count('ptmi_absmax'), out
    shared = packs()
    monkeypatch.setattr(tf, '_share_input', lambda x: x)
    apart = packs()
    assert apart[0] - shared[0] == 2 * 2 and apart[1] == shared[1] and torch.equal(shared[2], apart[2]), (shared[:2], apart[:2])


def test_strided_operands_give_the_bits_of_contiguous_copies():
    B, H, T, dh = 2, 3, TILE + 9, 16
    packed = rand(B, T, 3, H, dh, seed=1).to(DEV)                               # q | k | v side by side, heads innermost
    w = rand(B, H, T, dh, seed=2).to(DEV)

    def run(q, k, v, **kw):
        q, k, v = (t.detach().requires_grad_() for t in (q, k, v))
        out, weights = att().scaled_dot_product_attention(q, k, v, **kw)
        (out * w).sum().backward()
        return out.detach(), weights, q.grad, k.grad, v.grad
    for kw in (dict(bidirectional=True, seq_len=[T, 7]), dict(bidirectional=False)):
        views = [packed[:, :, i].transpose(1, 2) for i in range(3)]             # [B, H, T, dh] views of [B, T, (3,) H, dh]
        assert not views[0].is_contiguous()
        got = run(*views, **kw)
        want = run(*(t.contiguous() for t in views), **kw)
        for a, b in zip(got, want):
            assert torch.equal(a, b)
        # the projection output [B T, H dh] viewed as the reference views it
        flat = [t.transpose(1, 2).reshape(B * T, H * dh) for t in views]
        again = run(*(t.view(B, T, H, dh).transpose(1, 2) for t in flat), **kw)
        for a, b in zip(again, want):
            assert torch.equal(a, b)
        assert got[0].transpose(1, 2).is_contiguous()                           # out lies as [B, T, H, dh], ready for the out projection


def test_head_size_limit_and_cpu_tensors():
    q = torch.zeros(1, 1, 4, 129, device=DEV)
    with pytest.raises(NotImplementedError, match='128'):
        att().scaled_dot_product_attention(q, q, q)
    from padertorch_amd.contrib.je.modules import MultiHeadAttention
    mha = MultiHeadAttention(8, 8, 8, 258, 8, num_heads=2).to(DEV)
    with pytest.raises(NotImplementedError, match='128'):
        mha(torch.zeros(1, 3, 8, device=DEV), torch.zeros(1, 3, 8, device=DEV), torch.zeros(1, 3, 8, device=DEV))
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        att().scaled_dot_product_attention(torch.zeros(2, 3, 4), torch.zeros(2, 6, 4), torch.zeros(2, 6, 8))
    with pytest.raises(NotImplementedError):
        torch.ops.ptmi.attn_forward(torch.zeros(1, 1, 2, 4), torch.zeros(1, 1, 2, 4), torch.zeros(1, 1, 2, 4), None, False, None, 0.5)


# ------------------------------------------------------------------------------------------------ 2. glue
@pytest.mark.parametrize('T', [1, 37, 5000])
@pytest.mark.parametrize('d', [2, 6, 48])
def test_posenc(d, T):
    x = rand(2, T, d, seed=1)
    want = x.double() + ref.positional_encoding(T, d).double()
    leaf = x.to(DEV).requires_grad_()
    got = att().positional_encoding_(leaf * 1)
    w = rand(2, T, d, seed=2).to(DEV)
    (got * w).sum().backward()
    with Worst(f'posenc d={d} T={T}') as worst:
        worst.check('value', got, want, VALUE)
        assert torch.equal(leaf.grad, w)                             # the backward is the identity


@pytest.mark.parametrize('norm_first', [True, False])
@pytest.mark.parametrize('seq_len', [[37, 20, 1], None])
def test_norm_residual(norm_first, seq_len):
    from padertorch_amd.modules import Normalization
    B, T, N = 3, 37, 48
    z, res = rand(B, T, N, seed=1), rand(B, T, N, seed=2)
    gamma, beta, w = 1 + 0.3 * rand(1, 1, N, seed=3), 0.3 * rand(1, 1, N, seed=4), rand(B, T, N, seed=5)
    leaves64 = [t.double().requires_grad_() for t in (z, res, gamma, beta)]
    z64, r64, g64, b64 = leaves64
    want = (ref.masked_norm(z64, g64, b64, (2,), seq_len, 1e-2) + r64) if norm_first else ref.masked_norm(z64 + r64, g64, b64, (2,), seq_len, 1e-2)
    (want * w.double()).sum().backward()
    leaves = [t.to(DEV).requires_grad_() for t in (z, res, gamma, beta)]
    lengths = None if seq_len is None else torch.tensor(seq_len, dtype=torch.int32, device=DEV)
    got = att().norm_residual(*leaves, lengths, 1e-2, norm_first)
    (got * w.to(DEV)).sum().backward()
    with Worst(f'norm_residual norm_first={norm_first} seq_len={seq_len}') as worst:
        worst.check('value', got, want.detach(), VALUE)
        for name, a, b in zip(('dz', 'dres', 'dgamma', 'dbeta'), leaves, leaves64):
            worst.check(name, a.grad, b.grad, GRAD)
        # ... and it is what the Normalization module + add give
        norm = Normalization(data_format='btc', shape=(None, None, N), statistics_axis='c', eps=1e-2).to(DEV)
        with torch.no_grad():
            norm.gamma.copy_(gamma), norm.beta.copy_(beta)
            module = norm(z.to(DEV), seq_len) + res.to(DEV) if norm_first else norm(z.to(DEV) + res.to(DEV), seq_len)
        worst.check('against the module', got, module.double().cpu(), VALUE)
        if seq_len is not None:
            got64 = att().norm_residual(*(t.detach() for t in leaves), torch.tensor(seq_len, dtype=torch.int64, device=DEV), 1e-2, norm_first)
            assert torch.equal(got64, got)


# ------------------------------------------------------------------------------------------------ 3. the modules
def new_stack(g, name):
    from padertorch_amd.contrib.je.modules import TransformerLayerStack
    net = ref.variant_stack(g['variants'][name], TransformerLayerStack)
    net.load_state_dict(ref.state_dict_of(g, name), strict=True)
    return net.to(DEV).train()


def run_stack(net, g, name, seq_len='fixture'):
    cfg, x, m, state, w = ref.variant_inputs(g, name, torch.float32, DEV)
    for p in net.parameters():
        p.grad = None
    y, states = net(x, cfg['seq_len'] if seq_len == 'fixture' else seq_len, m=m, seq_len_m=cfg['seq_len_m'], state=state)
    (y * w).sum().backward()
    grads = {k: p.grad for k, p in net.named_parameters()}
    grads['x'] = x.grad
    if m is not None:
        grads['m'] = m.grad
    return y.detach(), [s.detach() for s in states], grads


@pytest.mark.parametrize('name', ['bi_nf', 'bi_nl', 'nonorm', 'batch', 'batch_b', 'cross', 'causal_state', 'causal_long'])
def test_stack_against_the_fixture(name):
    g = ref.golden()
    cfg = g['variants'][name]
    batch = cfg['norm'] == 'batch'

    def gate(base, key):
        return max(base, 4 * cfg['dev32'][key]) if batch else base
    y, states, grads = run_stack(new_stack(g, name), g, name)
    with Worst(f'stack {name}') as worst:
        worst.check('y', y, g[f'{name}/y64'], gate(VALUE, 'y'))                 # every position, padding included
        assert len(states) == 2
        for i, s in enumerate(states):
            worst.check(f'state {i}', s, g[f'{name}/out_state{i}'], gate(VALUE, f'out_state{i}'))
        assert sorted(grads) == sorted(cfg['names'])
        for k in cfg['names']:
            want = g[f'{name}/g64_{k}']
            if k in cfg['zero']:
                scale = float(abs(g[f'{name}/g64_{k[:-len("bias")]}weight']).max())
                worst.check(f'd{k} (analytically zero: absolute)', grads[k], want, GRAD, scale=scale)
            else:
                worst.check(f'd{k}', grads[k], want, gate(GRAD, 'g_' + k))
        if batch:
            # the gates used, where 4 x dev32 exceeds the project's (the analytically zero gradients are gated absolutely, above)
            used = {k: gate(GRAD if k.startswith('g_') else VALUE, k) for k in cfg['dev32'] if k[2:] not in cfg['zero']}
            wider = {k: v for k, v in used.items() if v not in (VALUE, GRAD)}
            with open(GATES, 'a') as f:
                f.write(f'stack {name}: gates max(project gate, 4 x dev32): y {used["y"]:.3g} (dev32 {cfg["dev32"]["y"]:.3g}), gradients '
                        f'{max(v for k, v in used.items() if k.startswith("g_")):.3g} at most; wider than the project gates: {wider or "none"}\n')


@pytest.mark.parametrize('num_heads', [4, 2])
def test_multi_head_attention_doctest_shapes(num_heads):
    from padertorch_amd.contrib.je.modules import MultiHeadAttention
    q, k, v, w = rand(2, 3, 4, seed=1), rand(2, 6, 6, seed=2), rand(2, 6, 8, seed=3), rand(2, 3, 4, seed=4)
    torch.manual_seed(7)
    mha = MultiHeadAttention(4, 6, 8, 4, 4, num_heads=num_heads)
    oracle = ref.MultiHeadAttention(4, 6, 8, 4, 4, num_heads=num_heads)
    oracle.load_state_dict(mha.state_dict(), strict=True)
    oracle.double()
    mha.to(DEV)
    with Worst(f'MultiHeadAttention doctest shapes, {num_heads} heads') as worst:
        for bidirectional, seq_len in ((False, None), (True, [6, 2])):
            mha.bidirectional = oracle.bidirectional = bidirectional
            leaves64 = [t.double().requires_grad_() for t in (q, k, v)]
            want, want_w = oracle(*leaves64, seq_len=seq_len)
            oracle.zero_grad()
            (want * w.double()).sum().backward()
            leaves = [t.to(DEV).requires_grad_() for t in (q, k, v)]
            mha.zero_grad()
            got, got_w = mha(*leaves, seq_len=seq_len)
            (got * w.to(DEV)).sum().backward()
            assert got.shape == (2, 3, 4) and got_w.shape == (2, num_heads, 3, 6)
            worst.check('y', got, want.detach(), VALUE)
            worst.check('weights', got_w, want_w.detach(), VALUE)
            for name, a, b in zip('qkv', leaves, leaves64):
                worst.check(f'd{name}', a.grad, b.grad, GRAD)
            for (n, p), p64 in zip(mha.named_parameters(), oracle.parameters()):
                if n == 'lin_key.bias':
                    worst.check(f'd{n} (absolute)', p.grad, p64.grad, GRAD, scale=float(oracle.lin_key.weight.grad.abs().max()))
                else:
                    worst.check(f'd{n}', p.grad, p64.grad, GRAD)
            assert mha(*leaves, seq_len=seq_len, need_weights=False)[1] is None


# ------------------------------------------------------------------------------------------------ 4. capture and determinism
def test_two_eager_runs_are_bit_identical():
    g = ref.golden()
    for name in ('bi_nf', 'cross', 'causal_state'):
        net = new_stack(g, name)
        y1, s1, g1 = run_stack(net, g, name)
        y2, s2, g2 = run_stack(net, g, name)
        assert torch.equal(y1, y2) and all(torch.equal(a, b) for a, b in zip(s1, s2))
        for k in g1:
            assert torch.equal(g1[k], g2[k]), (name, k)


def test_forward_backward_is_capturable_and_replays_bit_identically():
    g = ref.golden()
    name = 'bi_nf'
    net = new_stack(g, name)
    cfg, x0, _, _, w = ref.variant_inputs(g, name, torch.float32, DEV)
    params = list(net.parameters())
    inputs = [(x0.detach(), [37, 20, 1]), (rand(3, 37, 10, seed=11).to(DEV), [5, 37, 33]), (rand(3, 37, 10, seed=12).to(DEV), [37, 1, 20])]
    x = x0.detach().clone().requires_grad_()
    lengths = torch.tensor(inputs[0][1], dtype=torch.int32, device=DEV)

    def step():
        y, _ = net(x, lengths)
        return y, torch.autograd.grad((y * w).sum(), [x] + params)
    from padertorch_amd.ops import capture
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        step()                                              # eager warm-up on the capture stream (the positional table is made here)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with capture.capture_mode():
        with torch.cuda.graph(graph, stream=side):
            capture.zero_block(x.device)
            y_static, grads_static = step()
    for xin, lens in inputs[1:] + inputs[:1]:
        with torch.no_grad():
            x.copy_(xin)
            lengths.copy_(torch.tensor(lens, dtype=torch.int32))
        graph.replay()
        torch.cuda.synchronize()
        replayed = [y_static.clone()] + [t.clone() for t in grads_static]
        xe = xin.clone().requires_grad_()
        ye, _ = net(xe, torch.tensor(lens, dtype=torch.int32, device=DEV))
        eager = [ye.detach()] + list(torch.autograd.grad((ye * w).sum(), [xe] + params))
        for i, (a, b) in enumerate(zip(replayed, eager)):
            assert torch.equal(a, b), (lens, i)
