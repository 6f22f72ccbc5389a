"""Fast Griffin-Lim on the GPU against the reference's fp64 golden runs (tests/golden/g20_griffin_lim.npz).

Gates: one step is the project's STFT gates (1e-4 forward, 1e-4 inverse) taken together, 2e-4 max(a).  Behind that the iteration
amplifies rounding (about 5x per early iteration), so the gates of later iterations come from the deviation of the reference's OWN
fp32 run from its fp64 run (``dev32_n`` / ``devsig32_n`` in the golden): a differently ordered fp32 run is an independent draw of the
same amplified rounding and gets a factor 4.  Loss scalars (the RMSE history): 1e-4 relative."""
import contextlib

import numpy as np
import pytest
import torch

import griffin_lim_ref as ref

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
PLAN_CASES = ('s64', 's512', 's512w')        # register-FFT plans: both update paths; s40 takes the direct DFT and the composed path


def paths(case):
    return ('composed', 'fused') if case in PLAN_CASES else ('composed',)


ALL = [(c, p) for c in ref.CASES for p in paths(c)]


@contextlib.contextmanager
def options(path=None, poll=None):
    from padertorch_amd.ops import griffin_lim as gl
    before = gl.PATH, gl.POLL_EVERY
    if path is not None:
        gl.PATH = path
    if poll is not None:
        gl.POLL_EVERY = poll
    try:
        yield
    finally:
        gl.PATH, gl.POLL_EVERY = before


def setup(case, **kw):
    from padertorch_amd.ops import STFT
    g = ref.golden()
    st = STFT(**ref.stft_kwargs(g['geometries'][case]), **kw)
    a = torch.from_numpy(g[f'{case}_a']).to(DEV)
    x0 = torch.from_numpy(g[f'{case}_x0']).to(DEV)
    return g, st, a, x0


def run(case, iterations, atol=0., path=None, poll=None):
    from padertorch_amd.contrib.mk.synthesis import fast_griffin_lim
    g, st, a, x0 = setup(case)
    with options(path, poll):
        sig, info = fast_griffin_lim(a, st, alpha=float(g['alpha']), iterations=iterations, atol=atol, x=x0, return_info=True)
    return g, sig, info


def maxdev(got, want):
    got = got.detach().cpu().numpy() if isinstance(got, torch.Tensor) else got
    assert got.shape == want.shape, (got.shape, want.shape)
    assert np.all(np.isfinite(got))
    return float(np.max(np.abs(got - want)))


@pytest.mark.parametrize('case', ref.CASES)
def test_one_step(case):
    from padertorch_amd.contrib.mk.synthesis import griffin_lim_step
    g, st, a, x0 = setup(case)
    amax = float(g[f'{case}_a'].max())
    x1, audio = griffin_lim_step(a, x0, st)
    assert x1.dtype == torch.complex64 and audio.dtype == torch.float32
    assert audio.shape[-1] == g['geometries'][case]['samples']
    dev = maxdev(x1, g[f'{case}_x64_1']) / amax
    print(f'{case}: griffin_lim_step |x1 - x64_1| / max(a) = {dev:.3g}')
    assert dev <= 2e-4
    for p in paths(case):
        _, _, info = run(case, 1, path=p)
        dev = maxdev(info.x, g[f'{case}_x64_1']) / amax
        print(f'{case} {p}: iteration 1 |x - x64_1| / max(a) = {dev:.3g}')
        assert dev <= 2e-4
        assert int(info.num_iterations) == 1


def test_one_step_edge_bins():
    """Exact zeros in ``a``, exact zeros in ``y`` where ``a > 0`` and bins with ``|y|^2`` far below fp32's normal range."""
    from padertorch_amd.contrib.mk.synthesis import griffin_lim_step
    from padertorch_amd.ops import STFT
    from padertorch_amd.ops.griffin_lim import gl_project
    g = ref.golden()
    st = STFT(**ref.stft_kwargs(g['geometries']['edge']))
    a_np, y_np = g['edge_a'], g['edge_y']
    a, y = torch.from_numpy(a_np).to(DEV), torch.from_numpy(y_np).to(DEV)
    amax = float(a_np.max())
    P = torch.view_as_complex(gl_project(a, torch.view_as_real(y))).cpu().numpy()
    assert np.all(np.isfinite(P.view(np.float32)))
    dev = float(np.max(np.abs(P - g['edge_P64']))) / amax
    print(f'edge: |P - P64| / max(a) = {dev:.3g}')
    assert dev <= 2e-4
    flat, af = P.reshape(-1), a_np.reshape(-1)
    assert np.all(flat[g['edge_idx_a0']] == 0)                                                    # a == 0 -> 0
    assert np.all(flat[g['edge_idx_y0']].imag == 0) and np.all(flat[g['edge_idx_y0']].real == af[g['edge_idx_y0']])   # y == 0 -> (a, 0)
    tiny, want = flat[g['edge_idx_tiny']], af[g['edge_idx_tiny']].astype(np.float64) * np.sqrt(0.5)
    rel = max(float(np.max(np.abs(tiny.real - want) / want)), float(np.max(np.abs(tiny.imag - want) / want)))
    print(f'edge: denormal |y|^2 bins, relative deviation from a (sqrt 1/2, sqrt 1/2) = {rel:.3g}')
    assert rel <= 1e-6
    x1, audio = griffin_lim_step(a, y, st)
    dx, da = maxdev(x1, g['edge_x64']) / amax, maxdev(audio, g['edge_audio64']) / float(np.abs(g['edge_audio64']).max())
    print(f'edge: |x1 - x64| / max(a) = {dx:.3g}, |audio - audio64| / max|audio64| = {da:.3g}')
    assert dx <= 2e-4 and da <= 2e-4


@pytest.mark.parametrize('case,path', ALL)
def test_steps_2_and_3(case, path):
    g = ref.golden()
    amax = float(g[f'{case}_a'].max())
    for n in (2, 3):
        _, sig, info = run(case, n, path=path)
        gate = max(4 * float(g[f'{case}_dev32_{n}']), 2e-4)
        dev = maxdev(info.x, g[f'{case}_x64_{n}']) / amax
        print(f'{case} {path}: iteration {n} |x - x64| / max(a) = {dev:.3g} (gate {gate:.3g})')
        assert dev <= gate
    want = g[f'{case}_sig64_3']
    gate = max(4 * float(g[f'{case}_devsig32_3']), 2e-4)
    dev = maxdev(sig, want) / float(np.abs(want).max())
    print(f'{case} {path}: 3-iteration signal deviation {dev:.3g} (gate {gate:.3g})')
    assert dev <= gate


@pytest.mark.parametrize('case,path', ALL)
def test_30_iterations(case, path):
    from padertorch_amd.ops.griffin_lim import gl_project
    g, sig, info = run(case, 30, path=path)
    rmse = info.rmse.cpu().numpy().astype(np.float64)
    rel = float(np.max(np.abs(rmse - g[f'{case}_rmse64']) / g[f'{case}_rmse64']))
    print(f'{case} {path}: rmse history, worst relative deviation {rel:.3g}')
    assert int(info.num_iterations) == 30 and rel <= 1e-4
    want = g[f'{case}_sig64_30']
    gate = 4 * float(g[f'{case}_devsig32_30'])
    dev = maxdev(sig, want) / float(np.abs(want).max())
    print(f'{case} {path}: 30-iteration signal deviation {dev:.3g} (gate {gate:.3g})')
    assert dev <= gate
    a = torch.from_numpy(g[f'{case}_a']).to(DEV)
    final = torch.view_as_complex(gl_project(a, torch.view_as_real(info.x).contiguous()))
    rel = float(((final.abs() - a).abs() / a.clamp_min(1e-30)).max())
    print(f'{case} {path}: | |a exp(j angle x)| - a | / a = {rel:.3g}')
    assert rel <= 1e-6


@pytest.mark.parametrize('case', ['s64', 's512'])
def test_fused_against_composed(case):
    g = ref.golden()
    amax = float(g[f'{case}_a'].max())
    _, _, f3 = run(case, 3, path='fused')
    _, _, c3 = run(case, 3, path='composed')
    gate = max(4 * float(g[f'{case}_dev32_3']), 2e-4)
    dev = float((f3.x - c3.x).abs().max()) / amax
    print(f'{case}: fused vs composed, iteration 3: {dev:.3g} (gate {gate:.3g})')
    assert dev <= gate
    _, sf, f30 = run(case, 30, path='fused')
    _, sc, c30 = run(case, 30, path='composed')
    gate = 4 * float(g[f'{case}_devsig32_30'])
    dev = float((sf - sc).abs().max() / sc.abs().max())
    rel = float(((f30.rmse - c30.rmse).abs() / c30.rmse).max())
    print(f'{case}: fused vs composed, 30-iteration signal {dev:.3g} (gate {gate:.3g}), rmse histories {rel:.3g}')
    assert dev <= gate and rel <= 1e-4


@pytest.mark.parametrize('path', ['composed', 'fused'])
def test_stop(path):
    g = ref.golden()
    atol, k = float(g['stop_atol']), int(g['stop_k'])
    results = {}
    for poll in (0, 1, 8):
        _, sig, info = run('s64', 30, atol=atol, path=path, poll=poll)
        assert int(info.num_iterations) == k + 1, (poll, int(info.num_iterations), k)
        rmse = info.rmse.cpu().numpy()
        assert np.all(np.isfinite(rmse[:k + 1])) and np.all(np.isnan(rmse[k + 1:])), rmse
        assert rmse[k] < atol <= rmse[:k].min()
        results[poll] = (sig, info)
    want = g['stop_sig64']
    dev = maxdev(results[0][0], want) / float(np.abs(want).max())
    gate = 4 * float(g['s64_devsig32_30'])
    print(f'stop {path}: signal deviation {dev:.3g} (gate {gate:.3g})')
    assert dev <= gate
    for poll in (1, 8):       # the result does not depend on the host's polling
        assert torch.equal(results[poll][0], results[0][0]) and torch.equal(results[poll][1].x, results[0][1].x)
        assert torch.equal(results[poll][1].rmse.isnan(), results[0][1].rmse.isnan())
        assert torch.equal(results[poll][1].rmse[:k + 1], results[0][1].rmse[:k + 1])
    _, _, info = run('s64', 30, atol=0., path=path)
    assert int(info.num_iterations) == 30 and bool(torch.isfinite(info.rmse).all())


@pytest.mark.parametrize('path', ['composed', 'fused'])
def test_nan_input_runs_all_iterations(path):
    from padertorch_amd.contrib.mk.synthesis import fast_griffin_lim
    g, st, a, x0 = setup('s64')
    a = a.clone()
    a[0, 5, 7] = float('nan')
    with options(path, 2):
        sig, info = fast_griffin_lim(a, st, iterations=6, atol=0.1, x=x0, return_info=True)
    assert int(info.num_iterations) == 6
    assert bool(info.rmse.isnan().all()) and bool(sig.isnan().any())


def same(r1, r2):
    (s1, i1), (s2, i2) = r1, r2
    return (torch.equal(s1, s2) and torch.equal(torch.view_as_real(i1.x), torch.view_as_real(i2.x))
            and torch.equal(i1.rmse.isnan(), i2.rmse.isnan()) and torch.equal(i1.rmse.nan_to_num(-1.), i2.rmse.nan_to_num(-1.))
            and int(i1.num_iterations) == int(i2.num_iterations))


@pytest.mark.parametrize('path', ['composed', 'fused'])
def test_determinism_and_capture(path):
    from padertorch_amd.contrib.mk.synthesis import fast_griffin_lim
    g, st, a, x0 = setup('s64')
    atol, k = float(g['stop_atol']), int(g['stop_k'])

    def eager(a_, x0_):
        with options(path):
            return fast_griffin_lim(a_, st, iterations=30, atol=atol, x=x0_, return_info=True)

    inputs = {'loud': (10 * a, 10 * x0), 'golden': (a, x0)}     # 10 a: the RMSE never falls below the golden atol
    want = {name: eager(*io) for name, io in inputs.items()}
    assert int(want['loud'][1].num_iterations) == 30 and int(want['golden'][1].num_iterations) == k + 1
    assert same(eager(a, x0), want['golden'])                     # two eager runs: bit-identical
    a_s, x0_s = inputs['loud'][0].clone(), inputs['loud'][1].clone()
    graph = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with options(path):
        with torch.cuda.graph(graph):
            out = fast_griffin_lim(a_s, st, iterations=30, atol=atol, x=x0_s, return_info=True)
    for name in ('loud', 'golden', 'loud'):                      # a replay that stops early after one that did not, and back
        a_s.copy_(inputs[name][0])
        x0_s.copy_(inputs[name][1])
        graph.replay()
        torch.cuda.synchronize()
        assert same(out, want[name]), name


def test_iterations_0_and_its_gradient():
    from padertorch_amd.contrib.mk.synthesis import fast_griffin_lim
    g, st, a, x0 = setup('s64')
    a = a.clone().requires_grad_(True)
    sig, info = fast_griffin_lim(a, st, iterations=0, x=x0, return_info=True)
    assert info.rmse.numel() == 0 and int(info.num_iterations) == 0
    want = g['grad0_sig64']
    dev = maxdev(sig, want) / float(np.abs(want).max())
    (sig * torch.from_numpy(g['grad0_w']).to(DEV, torch.float32)).sum().backward()
    gdev = maxdev(a.grad, g['grad0_grad64']) / float(np.abs(g['grad0_grad64']).max())
    print(f'iterations=0: signal {dev:.3g}, gradient {gdev:.3g} (gates 2e-4)')
    assert dev <= 2e-4 and gdev <= 2e-4


def test_gradient_after_iterations_is_the_last_projection_only():
    """``a.requires_grad``: the gradient flows through the final projection and inverse; the phase is a constant."""
    from padertorch_amd.contrib.mk.synthesis import fast_griffin_lim
    from padertorch_amd.ops.griffin_lim import gl_project
    g, st, a, x0 = setup('s64')
    a1 = a.clone().requires_grad_(True)
    sig, info = fast_griffin_lim(a1, st, iterations=3, atol=0., x=x0, return_info=True)
    w = torch.from_numpy(g['grad0_w']).to(DEV, torch.float32)
    (sig * w).sum().backward()
    a2 = a.clone().requires_grad_(True)
    spec = torch.view_as_complex(gl_project(a2, torch.view_as_real(info.x).contiguous()))
    (st.inverse(spec) * w).sum().backward()
    assert torch.equal(a1.grad, a2.grad) and bool(a1.grad.abs().max() > 0)


def test_docstring_known_answer():
    """griffin_lim.py:88-100: a 200 Hz sine of 16000 samples, magnitudes (63, 513) -> signal (16128,)."""
    from padertorch_amd.contrib.mk.synthesis import fast_griffin_lim
    from padertorch_amd.ops import STFT
    t = np.linspace(0, 1, num=16000)
    sine = torch.from_numpy(np.sin(2 * np.pi * 200 * t).astype(np.float32)).to(DEV)
    st = STFT(1024, 256, window_length=None, window='hann', pad=True, fading='half')
    mag = st(sine).abs()
    assert tuple(mag.shape) == (63, 513)
    sig, info = fast_griffin_lim(mag, st, generator=torch.Generator(DEV).manual_seed(3), return_info=True)
    assert tuple(sig.shape) == (16128,) and bool(torch.isfinite(sig).all())
    rmse = info.rmse[:int(info.num_iterations)]
    assert float(rmse[-1]) < float(rmse[0])


def test_shapes_dtypes_and_representations():
    from padertorch_amd.contrib.mk.synthesis import FGLA, fast_griffin_lim
    from padertorch_amd.ops import STFT
    g, st, a, x0 = setup('s64')
    kw = dict(alpha=float(g['alpha']), iterations=5, atol=0.)
    a6, x6 = torch.cat([a, 2 * a, 3 * a]), torch.cat([x0, 2 * x0, 3 * x0])          # [6, frames, F]
    flat = fast_griffin_lim(a6, st, x=x6, **kw)
    lead = fast_griffin_lim(a6.reshape(2, 3, *a.shape[1:]), st, x=x6.reshape(2, 3, *a.shape[1:]), **kw)
    assert tuple(lead.shape) == (2, 3, flat.shape[-1]) and torch.equal(lead.reshape(6, -1), flat)
    s32 = fast_griffin_lim(a, st, x=x0, **kw)
    s64 = fast_griffin_lim(a.double(), st, x=x0, **kw)
    assert s64.dtype == torch.float64 and torch.equal(s64, s32.double())
    s16 = fast_griffin_lim(a.to(torch.bfloat16), st, x=x0, **kw)
    assert s16.dtype == torch.bfloat16
    for rep in ('stacked', 'concat'):
        st_r = STFT(**ref.stft_kwargs(g['geometries']['s64']), complex_representation=rep)
        assert torch.equal(fast_griffin_lim(a, st_r, x=x0, **kw), s32), rep
    gen = lambda seed: torch.Generator(DEV).manual_seed(seed)          # noqa: E731
    r1, r2, r3 = (fast_griffin_lim(a, st, generator=gen(s), **kw) for s in (11, 11, 12))
    assert torch.equal(r1, r2) and not torch.equal(r1, r3)
    fgla = FGLA(16000, st, alpha=0.9, iterations=4, atol=0.)
    torch.manual_seed(5)
    want = fast_griffin_lim(a, st, 0.9, 4, 0.)
    torch.manual_seed(5)
    assert torch.equal(fgla(a, sequence_lengths=[1, 2]), want)
    torch.manual_seed(5)
    assert torch.equal(fgla(g['s64_a'], target_sampling_rate=16000), want)        # a numpy spectrogram is moved to the GPU


def test_verbose_prints_the_history(capsys):
    _, st, a, x0 = setup('s64')
    from padertorch_amd.contrib.mk.synthesis import fast_griffin_lim
    fast_griffin_lim(a, st, iterations=3, atol=0., x=x0, verbose=True)
    lines = [line for line in capsys.readouterr().out.splitlines() if line.startswith('Reconstruction iteration')]
    assert len(lines) == 3 and lines[2].startswith('Reconstruction iteration: 2/3 RMSE: ')
