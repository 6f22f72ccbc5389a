"""The grouped planes GEMM (``ptmi_gemm_planes_bf16_group``: the products of two parts of A with up to three B segments in one launch
of the big-tile kernel and one slab reduction) against fp64 and against separate ``gemm_planes_bf16_`` calls, and the transposed bf16
pack of up to three sources in one launch (``ptmi_pack_planes_t_bf16_list``) against separate launches."""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'

#: (M, m_split, segment columns, K, split): a ragged last k range and columns ending inside a 16-wide fragment; K shorter than four
#: k blocks; the bottom BLSTM layer's tile geometry at a quarter of its K (more work items than CUs)
SHAPES = [(192, 96, (24, 40, 40), 333, 3), (320, 160, (257, 40, 40), 96, 1), (4800, 2400, (257, 600, 600), 2080, 8)]
#: a BLSTM layer's blocks (part * 3 + segment): (f, X), (f, H_f), (b, X), (b, H_b); (f, H_b) = 2 and (b, H_f) = 4 are skipped
BLOCKS = [0, 1, 3, 5]


@functools.lru_cache(maxsize=None)
def _case(shape):
    """Operands, their planes and the fp64 products of one shape (made once, read-only)."""
    M, m_split, ns, K, split = shape
    g = torch.Generator(device=DEV).manual_seed(M + K)
    a = torch.randn(K, M, device=DEV, generator=g) * 0.3
    xs = [torch.randn(K, n, device=DEV, generator=g) for n in ns]
    pa = torch.ops.ptmi.pack_planes_bf16(a, True)
    pbs = [torch.ops.ptmi.pack_planes_bf16(x, True) for x in xs]
    parts = [a[:, :m_split], a[:, m_split:]]
    want = {b: parts[b // 3].double().t() @ xs[b % 3].double() for b in BLOCKS}
    mag = {b: parts[b // 3].double().abs().t() @ xs[b % 3].double().abs() for b in BLOCKS}
    return pa, pbs, want, mag


def _buffers(shape, strided, seed=5):
    """Per part one buffer with the three blocks as column ranges behind each other (``strided``), or a buffer per block with three
    spare rows: ``(everything allocated, {block: view})``."""
    M, m_split, ns, K, split = shape
    g = torch.Generator(device=DEV).manual_seed(seed)
    rows = [m_split, M - m_split]
    views, bufs = {}, []
    for p in (0, 1):
        if strided:
            buf = torch.randn(rows[p] + 3, sum(ns) + 7, device=DEV, generator=g)
            bufs.append(buf)
            off = 0
            for s, n in enumerate(ns):
                views[p * 3 + s] = buf[:rows[p], off:off + n]
                off += n
        else:
            for s, n in enumerate(ns):
                buf = torch.randn(rows[p] + 3, n, device=DEV, generator=g)
                bufs.append(buf)
                views[p * 3 + s] = buf[:rows[p]]
    return bufs, views


@functools.lru_cache(maxsize=None)
def _separate(shape, acc, strided):
    """What separate ``gemm_planes_bf16_`` calls (cost model) leave in the same buffers."""
    from padertorch_amd import _lib
    M, m_split, ns, K, split = shape
    pa, pbs, _, _ = _case(shape)
    bufs, views = _buffers(shape, strided)
    half = int(_lib.load().ptmi_planes_elems(m_split, K)) * 2
    _lib.select_gemm_tile(-1)
    for b in BLOCKS:
        p, s = divmod(b, 3)
        torch.ops.ptmi.gemm_planes_bf16_(views[b], pa, p * half, pbs[s], None, (M - m_split) if p else m_split, ns[s], K, acc, split)
    torch.cuda.synchronize()
    return bufs


def _group(shape, views, acc):
    M, m_split, ns, K, split = shape
    pa, pbs, _, _ = _case(shape)
    return torch.ops.ptmi.gemm_planes_bf16_group_([views[b] for b in BLOCKS], BLOCKS, pa, 0, M, m_split, pbs, list(ns), K, acc, split)


@pytest.mark.parametrize('strided', [True, False])
@pytest.mark.parametrize('acc', [False, True])
@pytest.mark.parametrize('tile', [-1, 0, 1, 2, 3, 4])
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: f'{s[0]}x{"+".join(map(str, s[2]))}x{s[3]}')
def test_grouped_gemm_vs_fp64_and_separate_calls(shape, tile, acc, strided):
    from padertorch_amd import _lib
    from padertorch_amd.ops import gemm as G
    M, m_split, ns, K, split = shape
    _, _, want, mag = _case(shape)
    sep = _separate(shape, acc, strided)
    bufs, views = _buffers(shape, strided)
    before = [b.clone() for b in bufs]
    prior = {b: views[b].double().clone() for b in BLOCKS}
    _lib.select_gemm_tile(tile)
    try:
        plan = G.group_plan(M, m_split, list(ns), BLOCKS, K, split)
        ok = _group(shape, views, acc)
        torch.cuda.synchronize()
        assert ok == (plan // 100 != 5), (ok, plan)
        if tile >= 0:
            assert ok and plan == 100 * tile + min(split, (K + 31) // 32), plan          # a pinned tile takes split as it is
        if not ok:          # refused (the cost model prefers the 128 x 128 kernel for this shape): nothing was written
            assert all(torch.equal(x, y) for x, y in zip(bufs, before))
            return
        for b in BLOCKS:
            got = views[b].double()
            old = prior[b] if acc else 0
            err = float(((got - want[b] - old).abs() / (mag[b] + (prior[b].abs() if acc else 0))).max())
            print(f'block {b}: error / sum |a||b| = {err:.3g}')
            assert err < 8e-6, (b, err)          # bf16 (hi, lo) operands: 2^-17 per product
        # the separate calls: same buffers, same values to 1e-6 of the largest entry - outside the written blocks (spare rows, the
        # columns of the skipped blocks, the columns behind the last block) bit for bit what was there
        _, sep_views = _buffers_like(shape, strided, sep)
        for b in BLOCKS:          # (block by block: each against its own largest entry)
            d, big = float((views[b] - sep_views[b]).abs().max()), float(sep_views[b].abs().max())
            print(f'block {b}: |grouped - separate| = {d:.3g}, largest entry {big:.3g}')
            assert d <= 1e-6 * big, (b, d, big)
        keep = [torch.ones_like(b, dtype=torch.bool) for b in bufs]
        _, masks = _buffers_like(shape, strided, keep)
        for b in BLOCKS:
            masks[b].fill_(False)
        for x, z, k in zip(bufs, before, keep):
            assert torch.equal(x[k], z[k])
        # reproducible: the same call into fresh buffers gives the same bits
        bufs2, views2 = _buffers(shape, strided)
        assert _group(shape, views2, acc)
        torch.cuda.synchronize()
        assert all(torch.equal(x, y) for x, y in zip(bufs, bufs2))
    finally:
        _lib.select_gemm_tile(-1)


def _buffers_like(shape, strided, bufs):
    """The block views of :func:`_buffers` over the given tensors of the same shapes."""
    M, m_split, ns, K, split = shape
    rows = [m_split, M - m_split]
    views, it = {}, iter(bufs)
    for p in (0, 1):
        if strided:
            buf = next(it)
            off = 0
            for s, n in enumerate(ns):
                views[p * 3 + s] = buf[:rows[p], off:off + n]
                off += n
        else:
            for s, n in enumerate(ns):
                views[p * 3 + s] = next(it)[:rows[p]]
    return bufs, views


@pytest.mark.parametrize('tile', [-1, 3])
def test_grouped_gemm_refuses_a_part_boundary_inside_a_row_tile(tile):
    """m_split = 40 is no multiple of 16 (part 1's planes would not start at a row tile): refused, nothing launched."""
    from padertorch_amd import _lib
    from padertorch_amd.ops import gemm as G
    M, m_split, ns, K, split = 192, 40, (24, 40, 40), 333, 3
    g = torch.Generator(device=DEV).manual_seed(1)
    pa = torch.ops.ptmi.pack_planes_bf16(torch.randn(K, M, device=DEV, generator=g), True)
    pbs = [torch.ops.ptmi.pack_planes_bf16(torch.randn(K, n, device=DEV, generator=g), True) for n in ns]
    outs = [torch.randn((M - m_split) if b // 3 else m_split, ns[b % 3], device=DEV, generator=g) for b in BLOCKS]
    before = [o.clone() for o in outs]
    _lib.select_gemm_tile(tile)
    try:
        assert G.group_plan(M, m_split, list(ns), BLOCKS, K, split) // 100 == 5
        assert torch.ops.ptmi.gemm_planes_bf16_group_(outs, BLOCKS, pa, 0, M, m_split, pbs, list(ns), K, True, split) is False
        # the C entry itself: PTMI_E_UNSUPPORTED
        import ctypes
        lib = _lib.load()
        c = (ctypes.c_void_p * 6)()
        ldc = (ctypes.c_int64 * 6)()
        for o, b in zip(outs, BLOCKS):
            c[b], ldc[b] = o.data_ptr(), o.stride(0)
        n = (ctypes.c_int32 * 3)(*ns)
        ws = torch.empty(int(lib.ptmi_gemm_planes_group_workspace_elems(M, m_split, n, 3, c, K, split)), device=DEV)
        rc = lib.ptmi_gemm_planes_bf16_group(pa.data_ptr(), M, m_split, (ctypes.c_void_p * 3)(*[p.data_ptr() for p in pbs]), n, 3, c, ldc, K, 1,
                                             split, 3, ws.data_ptr(), _lib.stream(torch.device(DEV)))
        assert rc == -2, rc
        torch.cuda.synchronize()
        assert all(torch.equal(x, y) for x, y in zip(outs, before))
    finally:
        _lib.select_gemm_tile(-1)


@pytest.mark.parametrize('K,C,ld', [(8096, 2400, 4800), (1000, 514, 516), (70, 18, 20), (33, 257, 260), (5000, 1200, 1200)])
def test_pack_list_equals_separate_launches(K, C, ld):
    """Three sources in one launch - 16-byte aligned rows, the same values from a source shifted by one float (scalar loads), a column
    count that is no multiple of 16 - and one source alone: bit for bit the planes of ``pack_planes_bf16`` launches of their own."""
    torch.manual_seed(K + C)
    wide = torch.randn(K, ld, device=DEV)
    shifted = torch.zeros(K * ld + 1, device=DEV)[1:].view(K, ld)
    shifted.copy_(wide)
    c3 = C - 5 if (C - 5) % 16 else C - 6
    srcs = [wide[:, :C], shifted[:, :C], wide[:, :c3]]
    assert srcs[0].data_ptr() % 16 == 0 and srcs[1].data_ptr() % 16 != 0 and srcs[2].data_ptr() % 16 == 0 and c3 % 16 != 0
    want = [torch.ops.ptmi.pack_planes_bf16(s, True) for s in srcs]
    got = torch.ops.ptmi.pack_planes_bf16_list(srcs)
    assert len(got) == 3
    for g, w in zip(got, want):
        assert g.shape == w.shape and torch.equal(g.view(torch.int16), w.view(torch.int16))
    one = torch.ops.ptmi.pack_planes_bf16_list(srcs[2:])
    assert len(one) == 1 and torch.equal(one[0].view(torch.int16), want[2].view(torch.int16))
