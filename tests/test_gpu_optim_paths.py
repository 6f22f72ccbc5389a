"""The clip + Adam kernels (csrc/optim.hip) element by element against the fp64 restatement (oracle/optim_np.py) on every path of
``adam_flat_kernel``: float4 groups and the tail, groups that straddle segments, a full segment table, parameters at a storage offset
(the scalar branch for a pointer that is not 16-byte aligned), zero-element parameters, the grid-stride loop, hyper-parameters read
from device words, skipped updates; the optimizer wrapper on the same layouts; ``lstm_bias_grad_add_``.

The harness calls ``torch.ops.ptmi.adam_flat_`` / ``grad_norm`` directly and builds the segment table itself.  Every parameter is a view
into one sentinel-filled device buffer with at least 8 guard floats on each side, the flat g / m / v buffers have 8 guard floats behind
them, and every case requires all guard words bit-identical afterwards.

Measure and gate, per quantity ``q`` of p, m, v (tests/optim_paths_ref.py): ``err_q = max_i |q_i - q64_i| / terms_q,i`` over every
element, ``terms`` being the sum of the magnitudes that enter the element; ``gate_q = max(4 dev32_q, 4 * 2^-24)`` with ``dev32`` the
same measure of the restatement's own fp32 run (never of anything the kernels produce), plus 2e-7 (m, p) / 4e-7 (v) on clipped cases
for the kernels' own fp32 norm.  tests/test_oracle_optim.py holds dev32 <= 2^-17 on every input used here.  Each case prints err, dev32
and gate (profiles/optim_paths.txt holds a copy)."""
import numpy as np
import pytest
import torch

import optim_paths_ref as R

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
GUARD = 8
SENTINEL = -6.02e23
BETAS = (R.HYPER['beta1'], R.HYPER['beta2'])


@pytest.fixture(autouse=True)
def _registered_ops():
    import padertorch_amd.ops.library  # noqa: F401  (defines torch.ops.ptmi.*)


def bits(a):
    return np.ascontiguousarray(a).view(np.int32)


class Bucket:
    """Device state of one step: parameters scattered over a guarded arena, flat g / m / v with guard words behind, the segment table."""

    def __init__(self, layout, x):
        self.layout, self.n = layout, sum(n for n, _ in layout)
        starts, cur = [], 0
        for n, mis in layout:
            cur = (cur + GUARD + 3) // 4 * 4 + mis            # at least GUARD sentinels in front; address = mis floats (mod 4)
            starts.append(cur)
            cur += n
        total = (cur + GUARD + 3) // 4 * 4
        self.starts, self.offs = starts, R.flat_offsets(layout)
        arena = np.full(total, SENTINEL, np.float32)
        self.inside = np.zeros(total, bool)
        for s, o, (n, _) in zip(starts, self.offs, layout):
            arena[s:s + n] = x['p'][o:o + n]
            self.inside[s:s + n] = True
        assert self.inside.sum() == self.n
        self.arena0 = arena
        self.arena = torch.from_numpy(arena).to(DEV)
        assert self.arena.data_ptr() % 16 == 0
        self.params = [self.arena[s:s + n] for s, (n, _) in zip(starts, layout)]
        table = [(self.arena.data_ptr() + 4 * s, int(o), n) for s, o, (n, _) in zip(starts, self.offs, layout)]
        assert all(ptr % 16 == 4 * mis for (ptr, _, _), (_, mis) in zip(table, layout))
        self.segs = torch.tensor(table, dtype=torch.int64).to(DEV)
        self.flat0 = {k: np.concatenate([x[k], np.full(GUARD + (-self.n) % 4, SENTINEL, np.float32)]) for k in 'gmv'}
        self.flat = {k: torch.from_numpy(a).to(DEV) for k, a in self.flat0.items()}
        assert all(t.data_ptr() % 16 == 0 for t in self.flat.values())

    def view(self, k):
        return self.flat[k][:self.n]

    def set_grad(self, g):
        self.flat['g'][:self.n].copy_(torch.from_numpy(g))

    def step(self, t, wd, clipped, zero_grad, hyper=None, found_inf=None, finite=None, lr=R.HYPER['lr'], max_norm=R.MAX_NORM):
        """One call of the raw op; returns ``applied``."""
        norm = torch.ops.ptmi.grad_norm(self.view('g')) if clipped else None
        one = lambda v: None if v is None else torch.full((1,), v, dtype=torch.float32, device=DEV)            # noqa: E731
        applied = torch.ops.ptmi.adam_flat_(
            self.view('g'), self.view('m'), self.view('v'), self.segs, self.params, norm, float(max_norm if clipped else 1e10),
            one(found_inf), one(finite), torch.full((1,), float(t - 1), device=DEV), lr, R.HYPER['beta1'], R.HYPER['beta2'],
            R.HYPER['eps'], wd, zero_grad, hyper)
        torch.cuda.synchronize()
        return float(applied)

    def results(self):
        """``dict(p, m, v, g)`` on the host, after checking every guard word."""
        arena = self.arena.cpu().numpy()
        assert np.array_equal(bits(arena[~self.inside]), bits(self.arena0[~self.inside])), 'guard words around the parameters'
        out = dict(p=np.concatenate([arena[s:s + n] for s, (n, _) in zip(self.starts, self.layout)]))
        for k in 'gmv':
            a = self.flat[k].cpu().numpy()
            assert np.array_equal(bits(a[self.n:]), bits(self.flat0[k][self.n:])), f'guard words behind {k}'
            out[k] = a[:self.n]
        assert out['p'].size == self.n
        return out


def same_bits(a, b, quantities=R.QUANTITIES):
    return all(np.array_equal(bits(a[q]), bits(b[q])) for q in quantities)


def check(label, got, r64, dev32, gate):
    err = R.deviation(got, r64)
    for q in R.QUANTITIES:
        print(f'{label:36s} {q}  err {err[q] / R.EPS32:7.3f}  dev32 {dev32[q] / R.EPS32:7.3f}  gate {gate[q] / R.EPS32:7.3f}  (x 2^-24)')
    failed = [(q, err[q], gate[q]) for q in R.QUANTITIES if not err[q] <= gate[q]]
    assert not failed, (label, failed)


_CASES = {}


def case(key):
    """Inputs, the restatement and the kernels' results (``zero_grad`` on and off) of one (layout, t, weight decay, clip): once."""
    if key not in _CASES:
        name, t, wd, clipped = key
        x, r64, dev32, gate = R.reference(R.size(name), t, wd, clipped)
        runs = {}
        for zero_grad in (True, False):
            b = Bucket(R.LAYOUTS[name], x)
            applied = b.step(t, wd, clipped, zero_grad)
            runs[zero_grad] = dict(b.results(), applied=applied)
            del b
        _CASES[key] = dict(x=x, r64=r64, dev32=dev32, gate=gate, runs=runs)
    return _CASES[key]


@pytest.mark.parametrize('key', R.CASES, ids=R.case_id)
def test_step_against_the_restatement(key):
    name, t, wd, clipped = key
    c = case(key)
    x, zeroed, kept = c['x'], c['runs'][True], c['runs'][False]
    assert zeroed['applied'] == 1 and kept['applied'] == 1
    check(R.case_id(key), zeroed, c['r64'], c['dev32'], c['gate'])
    assert same_bits(zeroed, kept)                                              # zeroing the bucket changes nothing else
    assert not bits(zeroed['g']).any()                                          # all +0.0
    assert np.array_equal(bits(kept['g']), bits(x['g']))
    if wd == 0:
        assert np.array_equal(bits(zeroed['p'][:R.ZEROS]), bits(x['p'][:R.ZEROS]))
    assert not np.array_equal(zeroed['p'][R.ZEROS:], x['p'][R.ZEROS:])


def test_more_segments_than_the_table_holds_is_refused():
    """1025 segments through the raw op: PTMI_E_UNSUPPORTED, and nothing is launched."""
    n = sum(k for k, _ in R.TOO_MANY)
    x = R.inputs(n, 2)
    b = Bucket(R.TOO_MANY, x)
    assert b.segs.shape == (1025, 3)
    with pytest.raises(RuntimeError, match=r'ptmi_adam_flat.*code -2'):
        b.step(2, 0.01, True, True)
    torch.cuda.synchronize()
    got = b.results()
    assert same_bits(got, x, ('p', 'g', 'm', 'v'))


def hyper_words(lr, wd, max_norm):
    return torch.tensor([lr, R.HYPER['beta1'], R.HYPER['beta2'], R.HYPER['eps'], wd, max_norm, 0.0, 0.0], dtype=torch.float64, device=DEV)


@pytest.mark.parametrize('name', ['odd', 'big'])
def test_hyper_parameters_from_device_words(name):
    t, wd = 2, 0.01
    c = case((name, t, wd, True))
    words = hyper_words(R.HYPER['lr'], wd, R.MAX_NORM)
    b = Bucket(R.LAYOUTS[name], c['x'])
    # (by-value arguments of nonsense: the device words replace them)
    assert b.step(t, 77.0, True, True, hyper=words, lr=123.0, max_norm=0.0) == 1
    assert same_bits(b.results(), c['runs'][True])
    del b
    # other words in the same tensor: another learning rate, another clip value
    lr, max_norm = 3e-4, 0.25
    x, r64, dev32, gate = R.reference(R.size(name), t, wd, True, lr=lr, max_norm=max_norm)
    words[0], words[5] = lr, max_norm
    b = Bucket(R.LAYOUTS[name], x)
    assert b.step(t, 77.0, True, True, hyper=words, lr=123.0, max_norm=0.0) == 1
    got = b.results()
    check(f'{name} hyper lr {lr:g} max_norm {max_norm:g}', got, r64, dev32, gate)
    assert not same_bits(got, c['runs'][True], ('p',)) and not bits(got['g']).any()


@pytest.mark.parametrize('how', ['found_inf', 'nan_norm', 'inf_loss'])
def test_skipped_step_on_the_grid_stride_path(how):
    """The three ways a step is skipped, at the size where workgroups take a second trip: nothing but the bucket is written."""
    t, wd = 2, 0.01
    x = R.inputs(R.BIG_N, t)
    b = Bucket(R.LAYOUTS['big'], x)
    if how == 'nan_norm':
        b.view('g')[R.BIG_N - 1] = float('nan')                               # the tail element, past the last float4
    applied = b.step(t, wd, True, True, found_inf=1.0 if how == 'found_inf' else None,
                     finite=float('inf') if how == 'inf_loss' else None)
    assert applied == 0
    got = b.results()
    assert same_bits(got, x)
    assert not bits(got['g']).any()


# ---------------------------------------------------------------------------------------------------------------- the wrapper
def native(params, **kw):
    from padertorch_amd.train.optimizer import Adam
    opt = Adam(**kw)
    opt.set_parameters(params)
    opt.use_flat_grads()
    return opt


@pytest.mark.parametrize('count', [1024, 1025])
def test_wrapper_at_the_segment_limit(count):
    """1024 parameters run natively, 1025 stay on torch's Adam; both follow torch.optim.Adam on the CPU (the tolerances of
    test_gpu_optim.py::test_adam_matches_torch_cpu)."""
    W = R.WRAPPER
    init, grads = R.wrapper_draw(count)
    cpu = [torch.nn.Parameter(p.clone()) for p in init]
    gpu = [torch.nn.Parameter(p.clone().to(DEV)) for p in init]
    ref = torch.optim.Adam(cpu, lr=W['lr'], weight_decay=W['weight_decay'], foreach=False)
    opt = native(gpu, gradient_clipping=W['max_norm'], lr=W['lr'], weight_decay=W['weight_decay'])
    assert opt._native_ok() == (count <= 1024)
    for gs in grads:
        for p, q, g in zip(cpu, gpu, gs):
            p.grad = g.clone()
            q.grad.copy_(g)
        n_ref = torch.nn.utils.clip_grad_norm_(cpu, W['max_norm'])
        ref.step()
        n_got = opt.clip_grad()
        opt.step_and_zero_grad()
        assert abs(float(n_got) - float(n_ref)) <= 1e-6 * float(n_ref)
        assert float(opt.flat_grads.flat.abs().max()) == 0.0
        np.testing.assert_allclose(torch.cat([q.detach() for q in gpu]).cpu().numpy(), torch.cat([p.detach() for p in cpu]).numpy(),
                                   rtol=W['rtol'], atol=W['atol'])
    assert (opt._bound is not None) == (count <= 1024)                          # the native path bound the state, or never ran
    cat = lambda o, ps, k: torch.cat([o.state[p][k].reshape(-1) for p in ps]).cpu().numpy()                     # noqa: E731
    assert all(float(opt.optimizer.state[q]['step']) == 3 for q in gpu)
    np.testing.assert_allclose(cat(opt.optimizer, gpu, 'exp_avg'), cat(ref, cpu, 'exp_avg'), rtol=2e-6, atol=1e-9)
    np.testing.assert_allclose(cat(opt.optimizer, gpu, 'exp_avg_sq'), cat(ref, cpu, 'exp_avg_sq'), rtol=2e-6, atol=1e-12)


OFFSET_SHAPES = [(37, 29), (513,), (3, 5, 7), (1,), (1200,), (6,), (2, 255)]


def offset_model(x):
    """Parameters that are contiguous views 1, 2, 3, ... floats into allocations of their own; ``(parameters, allocations, slices)``."""
    params, allocs, where, off = [], [], [], 0
    for i, shape in enumerate(OFFSET_SHAPES):
        n, k = int(np.prod(shape)), 1 + i % 3
        buf = torch.full((n + 2 * GUARD,), SENTINEL, device=DEV)
        buf[k:k + n] = torch.from_numpy(x['p'][off:off + n]).to(DEV)
        params.append(torch.nn.Parameter(buf[k:k + n].view(shape)))
        assert params[-1].data_ptr() == buf.data_ptr() + 4 * k and params[-1].is_contiguous()
        allocs.append(buf)
        where.append((k, n))
        off += n
    return params, allocs, where


def test_wrapper_trains_parameters_at_a_storage_offset():
    """A model whose parameters are offset views passes ``_native_ok()``: two steps, each gated from the state the GPU held before it."""
    n, wd = sum(int(np.prod(s)) for s in OFFSET_SHAPES), 0.01
    x = R.inputs(n, 1)
    params, allocs, where = offset_model(x)
    opt = native(params, gradient_clipping=R.MAX_NORM, lr=R.HYPER['lr'], betas=BETAS, eps=R.HYPER['eps'], weight_decay=wd)
    assert opt._native_ok()
    flat = lambda ts: torch.cat([a.detach().reshape(-1) for a in ts]).cpu().numpy()                            # noqa: E731
    state = dict(p=x['p'], m=np.zeros(n, np.float32), v=np.zeros(n, np.float32))
    for t in (1, 2):
        g = R.inputs(n, t)['g']
        opt.flat_grads.flat.copy_(torch.from_numpy(g))
        assert all(q.grad.data_ptr() == opt.flat_grads.flat.data_ptr() + 4 * o for q, o in zip(params, np.cumsum([0] + [k for _, k in where])))
        opt.clip_grad()
        opt.step_and_zero_grad()
        kw = dict(R.HYPER, weight_decay=wd, max_norm=R.MAX_NORM)
        r64 = R.optim_np.clip_adam_step(state['p'], g, state['m'], state['v'], t, **kw)
        r32 = R.optim_np.clip_adam_step(state['p'], g, state['m'], state['v'], t, dtype=np.float32, **kw)
        dev32 = R.deviation(r32, r64)
        got = dict(p=flat(params), m=flat([opt.optimizer.state[q]['exp_avg'] for q in params]),
                   v=flat([opt.optimizer.state[q]['exp_avg_sq'] for q in params]))
        check(f'wrapper, offset views, t {t}', got, r64, dev32, R.gates(dev32, True))
        assert all(float(opt.optimizer.state[q]['step']) == t for q in params)
        assert float(opt.flat_grads.flat.abs().max()) == 0.0
        state = got
    for buf, (k, m) in zip(allocs, where):
        rest = torch.cat([buf[:k], buf[k + m:]]).cpu().numpy()
        assert np.array_equal(bits(rest), bits(np.full(rest.size, SENTINEL, np.float32)))


def test_wrapper_with_zero_element_parameters_keeps_its_binding():
    """Zero-element parameters (their ``data_ptr()`` is null) train natively, follow torch on the CPU, and the flat moments bound at the
    first step are the ones every later step finds."""
    gen = torch.Generator().manual_seed(7)
    shapes = [(0,), (5, 3), (0, 4), (0,), (33,), (0,)]
    cpu = [torch.nn.Parameter(torch.randn(s, generator=gen)) for s in shapes]
    gpu = [torch.nn.Parameter(p.detach().clone().to(DEV)) for p in cpu]
    ref = torch.optim.Adam(cpu, lr=1e-3, foreach=False)
    opt = native(gpu, gradient_clipping=0.5, lr=1e-3)
    assert opt._native_ok()
    bound = None
    for step in range(3):
        for p, q in zip(cpu, gpu):
            p.grad = torch.randn(p.shape, generator=gen)
            q.grad.copy_(p.grad)
        torch.nn.utils.clip_grad_norm_(cpu, 0.5)
        ref.step()
        opt.clip_grad()
        opt.step_and_zero_grad()
        bound = bound or opt._bound
        assert opt._bound is bound, step
        for p, q in zip(cpu, gpu):
            np.testing.assert_allclose(q.detach().cpu().numpy(), p.detach().numpy(), rtol=2e-6, atol=2e-7)
    assert all(float(opt.optimizer.state[q]['step']) == 3 for q in gpu)


def test_wrapper_device_hyper_follows_a_changed_learning_rate():
    """``refresh_device_hyper()`` + ``hyper_from_device``: the learning rate halved between two eager steps gives the bits of two by-value
    steps with those learning rates - and it is the device words the kernel reads, not ``param_groups``."""
    n = sum(int(np.prod(s)) for s in OFFSET_SHAPES)
    x = R.inputs(n, 1)
    out = {}
    for how in ('value', 'device'):
        params, _, _ = offset_model(x)
        opt = native(params, gradient_clipping=R.MAX_NORM, lr=1e-3, weight_decay=0.01)
        group = opt.optimizer.param_groups[0]
        if how == 'device':
            opt.refresh_device_hyper()
            opt.hyper_from_device = True
        for t in (1, 2):
            opt.flat_grads.flat.copy_(torch.from_numpy(R.inputs(n, t)['g']))
            if t == 2:
                group['lr'] = 5e-4
                if how == 'device':
                    words = opt.refresh_device_hyper()
                    assert float(words[0]) == 5e-4
                    group['lr'] = 123.0                                         # not refreshed: the step must not see it
            opt.clip_grad()
            opt.step_and_zero_grad()
        out[how] = [q.detach().clone() for q in params] + [opt.optimizer.state[q][k].clone() for q in params for k in ('exp_avg', 'exp_avg_sq')]
    assert all(torch.equal(a, b) for a, b in zip(out['value'], out['device']))
    assert not torch.equal(out['value'][1].cpu(), torch.from_numpy(x['p'][37 * 29:37 * 29 + 513]))           # and the steps were taken


# ---------------------------------------------------------------------------------------------------------------- lstm_bias_grad_add_
@pytest.mark.parametrize('n', [1, 255, 256, 257, 2400])
@pytest.mark.parametrize('ndir', [1, 2])
def test_lstm_bias_grad_add(ndir, n):
    """``bias_ih.grad[d] += db[d]; bias_hh.grad[d] += db[d]``: one fp32 add has one rounding, so torch's own add gives the same bits."""
    gen = torch.Generator().manual_seed(1000 * ndir + n)
    stride = (n + 2 * GUARD + 3) // 4 * 4
    arena = torch.full((2 * ndir * stride,), SENTINEL, device=DEV)
    views = [arena[i * stride + GUARD:i * stride + GUARD + n] for i in range(2 * ndir)]           # [ih 0, hh 0, ih 1, hh 1]
    for v in views:
        v.copy_(torch.randn(n, generator=gen) * 10.0 ** torch.randint(-3, 3, (n,), generator=gen))
    db = torch.cat([torch.randn(ndir, n, generator=gen).reshape(-1), torch.full((GUARD,), SENTINEL)]).to(DEV)
    before = arena.clone()
    want = [v + db[:ndir * n].view(ndir, n)[i // 2] for i, v in enumerate(views)]
    torch.ops.ptmi.lstm_bias_grad_add_(db[:ndir * n].view(ndir, n), views[0::2], views[1::2])
    torch.cuda.synchronize()
    for i, v in enumerate(views):
        assert torch.equal(v, want[i]), i
    assert not torch.equal(arena, before)
    mask = torch.ones_like(arena, dtype=torch.bool)
    for i in range(2 * ndir):
        mask[i * stride + GUARD:i * stride + GUARD + n] = False
    assert torch.equal(arena[mask], before[mask])
    assert torch.equal(db[ndir * n:], torch.full((GUARD,), SENTINEL, device=DEV))
