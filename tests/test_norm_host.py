"""Masked normalisation (``csrc/norm.hip`` through ``modules.normalize``) without a GPU: the case table and the input generator that
``tests/test_gpu_norm_paths.py`` and ``tests/test_oracle_norm.py`` import from here, and the proof that the table reaches every
reduction path of ``ptmi_norm_reduce`` - asked of the library's own planner (``ptmi_norm_workspace_elems``), not of a copy of it.

Paths of ``ptmi_norm_reduce``.  A reduction has ``n_groups`` outputs and ``n_red`` reduced elements per output; ``which = 0`` reduces
over the statistics axes (modes 0 and 1: statistics and backward statistics), ``which = 1`` over the axes gamma / beta are broadcast
along (mode 2: their gradients).  The group tile ``gt`` is 1 when the innermost axis (of size > 1) is reduced or there is one group
(lanes along the reduction, wave shuffle + LDS), else 64 (a 64 x 4 thread layout, column sum in LDS; the last tile is partial when
``n_groups % 64 != 0``).  ``plan_chunks`` cuts the reduced range into ``nchunks`` workgroups; ``norm_reduce2_kernel`` folds them one
thread per output for ``nchunks <= 8`` and one wavefront per output above.  The workspace holds ``3 n_groups nchunks`` doubles, which
is how ``nchunks`` is read here.  ``ptmi_norm_elementwise`` becomes a grid-stride loop above 4096 x 256 elements.

Out of scope: the ``long long`` index instantiations of both kernels, taken from 2^31 - 1 elements on, need an 8 GiB float32 tensor
(and as much again for every result); no test here or in the GPU file reaches them.
"""
import numpy as np
import pytest

EPS = 1e-5
GRID_STRIDE_ABOVE = 4096 * 256


def _case(name, fmt, shape, stat, indep, lens, shift=True, scale=True, view=None, loss='w'):
    """``stat`` / ``indep``: axis letters of ``fmt`` (``indep`` None: no gamma / beta); ``view='transposed'``: x arrives as a
    non-contiguous view (its last two axes swapped in memory); ``loss='sum'``: the loss is ``y.sum()``, grad_y arrives expanded."""
    ax = {c: i for i, c in enumerate(fmt)}
    return dict(name=name, shape=shape, stat=tuple(ax[c] for c in stat), indep=None if indep is None else tuple(ax[c] for c in indep),
                batch_axis=ax['b'], sequence_axis=ax['t'], lens=lens, shift=shift, scale=scale, view=view, loss=loss)


CASES = [
    # ---- innermost axis kept: gt = 64 -----------------------------------------------------------------------------------------------
    _case('btf t-f one chunk', 'btf', (2, 20, 70), 't', 'f', [20, 7], view='transposed'),
    _case('btf t-f few chunks', 'btf', (5, 100, 129), 't', 'f', [100, 64, 33, 100, 1]),
    _case('btf t-f model layout', 'btf', (3, 230, 70), 't', 'f', [230, 117, 9]),
    _case('tbf tb-f', 'tbf', (90, 4, 65), 'tb', 'f', [90, 41, 90, 5]),
    _case('btf bt-f one partial tile', 'btf', (3, 50, 33), 'bt', 'f', [50, 50, 17]),
    _case('btf t-f F=1', 'btf', (4, 70, 1), 't', 'f', [70, 33, 1, 12]),
    _case('rank 5', 'bactf', (2, 2, 3, 50, 33), 'at', 'f', [50, 21]),
    _case('btf t-f grid stride', 'btf', (8, 520, 257), 't', 'f', [520, 333, 1, 64, 257, 519, 100, 520]),
    # ---- innermost axis reduced: gt = 1 ---------------------------------------------------------------------------------------------
    _case('bct t-c many chunks', 'bct', (2, 3, 5000), 't', 'c', [5000, 2601]),
    _case('bct t-c shift only', 'bct', (2, 3, 1500), 't', 'c', [1500, 700], scale=False),
    _case('bct bt-c', 'bct', (4, 5, 600), 'bt', 'c', [600, 311, 77, 600]),
    _case('bcft bft-c', 'bcft', (2, 3, 9, 130), 'bft', 'c', [130, 61]),
    _case('bct t-c one chunk, a length of 0', 'bct', (3, 3, 100), 't', 'c', [100, 0, 37]),
    _case('bcft bft-c F=1, no lengths', 'bcft', (3, 4, 1, 64), 'bft', 'c', None),
    _case('btf f-none scale only, y.sum()', 'btf', (3, 40, 257), 'f', None, [40, 13, 40], shift=False, loss='sum'),
]
BY_NAME = {c['name']: c for c in CASES}
NAMES = list(BY_NAME)
assert len(NAMES) == len(CASES)


def affine_shape(c):
    return None if c['indep'] is None else tuple(s if d in c['indep'] else 1 for d, s in enumerate(c['shape']))


def make_inputs(c, seed=0):
    """float32 ``x = 1.5 + 3 randn`` (a mean comparable to the spread: float32 rounding of the mean does not dominate the centred
    values), cotangent ``w`` (ones for ``loss='sum'``), ``gamma = 1 + 0.5 randn`` with scale, ``beta = 0.5 randn`` with shift."""
    rng = np.random.default_rng([seed, NAMES.index(c['name'])])
    x = (1.5 + 3 * rng.standard_normal(c['shape'])).astype(np.float32)
    w = rng.standard_normal(c['shape']).astype(np.float32)
    if c['loss'] == 'sum':
        w = np.ones(c['shape'], np.float32)
    gamma = beta = None
    if c['indep'] is not None and c['scale']:
        gamma = (1 + 0.5 * rng.standard_normal(affine_shape(c))).astype(np.float32)
    if c['indep'] is not None and c['shift']:
        beta = (0.5 * rng.standard_normal(affine_shape(c))).astype(np.float32)
    return dict(x=x, w=w, gamma=gamma, beta=beta)


def oracle_args(c):
    """The arguments ``oracle.norm_np.normalize`` and ``modules.normalize`` share after ``(x, gamma, beta)``."""
    return c['stat'], c['batch_axis'], c['sequence_axis'], c['lens'], c['shift'], c['scale'], EPS


# ---- which path a case takes, by the library's planner --------------------------------------------------------------------------------
def plan(c, which):
    """``dict(gt, n_groups, n_red, tiles, last_tile, nchunks)`` of the reduction ``which`` (0 statistics, 1 affine; None without
    gamma / beta): the geometry ``modules.normalize`` hands the library, ``nchunks`` from its workspace query."""
    from padertorch_amd import _lib
    from padertorch_amd.modules.normalization import _geometry
    if which == 1 and c['indep'] is None:
        return None
    shape = c['shape']
    geom, _, n_stat = _geometry(shape, c['stat'], affine_shape(c), c['batch_axis'], c['sequence_axis'])
    stride = geom.stat_group_stride if which == 0 else geom.indep_stride
    kept = [d for d in range(len(shape)) if stride[d] != 0 or shape[d] == 1]
    n_groups = int(np.prod([shape[d] for d in kept], dtype=np.int64))
    n_red = int(np.prod(shape, dtype=np.int64)) // n_groups
    if which == 0:
        assert n_groups == n_stat
    inner_reduced = (len(shape) - 1) not in kept
    gt = 1 if inner_reduced or n_groups == 1 else 64
    elems = int(_lib.load().ptmi_norm_workspace_elems(geom, which))
    assert elems > 0 and elems % (3 * n_groups) == 0, (c['name'], which, elems, n_groups)
    return dict(gt=gt, n_groups=n_groups, n_red=n_red, tiles=-(-n_groups // gt), last_tile=n_groups % gt or gt,
                nchunks=elems // (3 * n_groups))


def path_classes(p):
    """The classes of the coverage proof a planned reduction falls into."""
    if p is None:
        return set()
    fold = 'one chunk' if p['nchunks'] == 1 else 'thread fold' if p['nchunks'] <= 8 else 'wavefront fold'
    out = {f'gt={p["gt"]}, {fold}'}
    if p['gt'] == 64 and p['last_tile'] != 64:
        out.add('gt=64, several tiles, last partial' if p['tiles'] > 1 else 'gt=64, a single partial tile')
    return out


def describe(c):
    """One line for the printed tables: what each reduction of the case runs as."""
    def one(p):
        if p is None:
            return '-'
        tiles = f', {p["tiles"]} tile(s), last of {p["last_tile"]}' if p['gt'] == 64 else ''
        return f'gt {p["gt"]}, {p["nchunks"]} chunk(s) of {p["n_groups"]} x {p["n_red"]}{tiles}'
    n = int(np.prod(c['shape']))
    return f'stats {one(plan(c, 0))}; affine {one(plan(c, 1))}; elementwise {"grid-stride" if n > GRID_STRIDE_ABOVE else "one pass"}'


WANTED = {f'gt={gt}, {fold}' for gt in (1, 64) for fold in ('one chunk', 'thread fold', 'wavefront fold')} | {
    'gt=64, several tiles, last partial', 'gt=64, a single partial tile'}


@pytest.mark.parametrize('which', [0, 1], ids=['statistics (modes 0, 1)', 'affine (mode 2)'])
def test_the_table_reaches_every_class_of_the_reduction(which):
    reached = {}
    for c in CASES:
        for k in path_classes(plan(c, which)):
            reached.setdefault(k, []).append(c['name'])
    print()
    for k in sorted(WANTED):
        print(f'{k}: {reached.get(k, [])}')
    assert not WANTED - set(reached), sorted(WANTED - set(reached))


def test_every_case_keeps_the_class_it_was_chosen_for():
    """A change to ``plan_chunks`` that moves a case shows here by name (the class test above then says what is no longer reached)."""
    print()
    for c in CASES:
        print(f'{c["name"]} {c["shape"]}: {describe(c)}')
    want = {   # (statistics, affine): (gt, fold)
        'btf t-f one chunk': ((64, 'one chunk'), (64, 'one chunk')),
        'btf t-f few chunks': ((64, 'thread fold'), (64, 'wavefront fold')),
        'btf t-f model layout': ((64, 'wavefront fold'), (64, 'wavefront fold')),
        'tbf tb-f': ((64, 'wavefront fold'), (64, 'wavefront fold')),
        'btf bt-f one partial tile': ((64, 'thread fold'), (64, 'thread fold')),
        'rank 5': ((64, 'thread fold'), (64, 'wavefront fold')),
        'bct t-c many chunks': ((1, 'wavefront fold'), (1, 'wavefront fold')),
        'bct t-c shift only': ((1, 'thread fold'), (1, 'thread fold')),
        'bct bt-c': ((1, 'thread fold'), (1, 'thread fold')),
        'bcft bft-c': ((1, 'thread fold'), (1, 'thread fold')),
        'bct t-c one chunk, a length of 0': ((1, 'one chunk'), (1, 'one chunk')),
    }
    for name, folds in want.items():
        for which, (gt, fold) in enumerate(folds):
            assert f'gt={gt}, {fold}' in path_classes(plan(BY_NAME[name], which)), (name, which, plan(BY_NAME[name], which))
    # the 64 x 4 layout's tiles
    assert plan(BY_NAME['btf t-f one chunk'], 0)['tiles'] == 3 and plan(BY_NAME['btf t-f one chunk'], 0)['last_tile'] == 140 % 64
    assert (plan(BY_NAME['tbf tb-f'], 1)['tiles'], plan(BY_NAME['tbf tb-f'], 1)['last_tile']) == (2, 1)
    assert (plan(BY_NAME['rank 5'], 1)['tiles'], plan(BY_NAME['rank 5'], 1)['last_tile']) == (1, 33)
    assert (plan(BY_NAME['btf bt-f one partial tile'], 0)['tiles'], plan(BY_NAME['btf bt-f one partial tile'], 0)['last_tile']) == (1, 33)
    # an innermost axis of size 1 counts as kept: four groups on the 64 x 4 layout, strided reads
    assert plan(BY_NAME['btf t-f F=1'], 0)['gt'] == 64 and plan(BY_NAME['btf t-f F=1'], 0)['n_groups'] == 4
    # one group only: lanes along the reduction whatever the innermost axis
    assert plan(BY_NAME['btf f-none scale only, y.sum()'], 1) is None


def test_the_table_has_the_sizes_and_variants_the_kernels_branch_on():
    sizes = [int(np.prod(c['shape'])) for c in CASES]
    assert sum(n > GRID_STRIDE_ABOVE for n in sizes) == 1 and max(sizes) < 1.1 * GRID_STRIDE_ABOVE     # one, and no larger than needed
    assert any(len(c['shape']) == 5 for c in CASES)
    assert any(c['lens'] is None for c in CASES) and any(c['lens'] and 0 in c['lens'] for c in CASES)
    assert any(1 in c['shape'][1:-1] for c in CASES)                                                       # a size-1 axis in the middle
    assert any(c['view'] == 'transposed' for c in CASES) and any(c['loss'] == 'sum' for c in CASES)
    axis_sizes = {s for c in CASES for s in c['shape']}
    assert {1, 2, 3, 4, 5, 33, 64, 65, 129, 257} <= axis_sizes                                           # both sides of powers of two
    assert {(c['shift'], c['scale']) for c in CASES} == {(True, True), (True, False), (False, True)}
    for c in CASES:
        assert c['lens'] is None or (len(c['lens']) == c['shape'][c['batch_axis']] and max(c['lens']) <= c['shape'][c['sequence_axis']])


def test_no_group_of_a_gradient_case_has_constant_input():
    """Where ``power - mean^2`` is clamped at 0 the hand-written backward (like the reference's) ignores the clamp and autograd does
    not.  No group here comes near it: of every group with at least two values the variance is a sizeable part of its power.  (A group
    of one value or none has ``x - mean = 0`` exactly and zero gradients either way.)"""
    from oracle import norm_np as N
    for c in CASES:
        i = make_inputs(c)
        _, mean, power, n = N.normalize(i['x'], i['gamma'], i['beta'], *oracle_args(c))
        several = n >= 2
        assert several.any()
        if c['shift']:
            assert ((power - mean ** 2)[several] > 0.05 * power[several]).all(), c['name']
        assert (power[several] > 0.1).all(), c['name']
