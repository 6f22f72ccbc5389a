"""The contract of ptmi_lstm_forward_persistent / ptmi_lstm_backward_persistent (the tables in include/ptmi.h): every refusal
comes with its code and with NOTHING enqueued - the scratch, which an accepted call's first launch fills, keeps its contents.

Every argument of every call, the offending one included, is a real device buffer large enough for the shape the call names (all
are sized for the largest shape used here), so a check that went missing would show as a wrong return code, not as a stray access.
Of the last row of the backward table (H % 4, a plan that is not supported, more than 2^31 bytes) the first two are triggered; the
third would need buffers of 2 GiB each."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
T, B, H, NDIR = 3, 16, 8, 2
B_MAX, ND_MAX, KP_MAX = 80, 3, 32          # the largest batch (more than 64 row slots), direction count and KP a case names
SENTINEL = 0x5A5A5A5A
OK, INVALID, UNSUPPORTED = 0, -1, -2


def _meta(batch_sizes):
    from padertorch_amd.ops import lstm as L
    return L.pack_meta(torch.tensor(batch_sizes, dtype=torch.int64), torch.device(DEV))


class _Buffers:
    def __init__(self, lib):
        rows = T * B_MAX
        f32 = dict(dtype=torch.float32, device=DEV)
        torch.manual_seed(0)
        self.gates = torch.rand(rows, ND_MAX * 4 * H, **f32)
        self.hy = torch.zeros(rows, ND_MAX * H, **f32)
        self.c = torch.randn(rows, ND_MAX * H, **f32)
        self.dhy = torch.randn(rows, ND_MAX * H, **f32)
        self.c0 = torch.randn(ND_MAX, B_MAX, H, **f32)
        self.dc_n = torch.randn(ND_MAX, B_MAX, H, **f32)
        self.carry = torch.zeros(ND_MAX, B_MAX, H, **f32)
        self.w_pad = torch.randn(ND_MAX, 4 * H, KP_MAX, **f32) * 0.1
        self.w_t = torch.randn(ND_MAX, H, 4 * H, **f32) * 0.1
        self.dg = torch.zeros(rows, ND_MAX * 4 * H, **f32)
        self.planes = torch.zeros(ND_MAX * int(lib.ptmi_planes_elems(4 * H, rows)) + 8, dtype=torch.bfloat16, device=DEV)
        self.masks = torch.tensor([[0xFFFF, 0xFFFF if t == 0 else 0, 0xFFFF if t == T - 1 else 0] for t in range(T)],
                                  dtype=torch.int64, device=DEV)
        self.scratch = {back: torch.empty(int(lib.ptmi_lstm_scratch_elems(T, ND_MAX, B_MAX, H, back)), dtype=torch.int32, device=DEV)
                        for back in (0, 1)}
        self.metas = {'equal': _meta([B] * T), 'ragged': _meta([B, B, B - 1]), 'b24': _meta([24] * T), 'b80': _meta([B_MAX] * T)}

    def arm(self):
        for s in self.scratch.values():
            s.fill_(SENTINEL)

    def untouched(self):
        torch.cuda.synchronize()
        return all(bool((s == SENTINEL).all()) for s in self.scratch.values())


def _run(lib, buf, call, cases, monkeypatch):
    for name, over, want in cases:
        buf.arm()
        if over.pop('f32', False):
            monkeypatch.setenv('PTMI_LSTM_F32', '1')
        rc = call(**over)
        monkeypatch.delenv('PTMI_LSTM_F32', raising=False)
        assert rc == want, (name, rc, want)
        assert buf.untouched(), f'{name}: refused, but the scratch was written'
    buf.arm()
    assert call() == OK                 # ... and the call these cases vary is one the library runs: it writes its scratch
    assert not buf.untouched()
    from padertorch_amd.ops import lstm as L
    L.check_errors()


def test_backward_refusals(monkeypatch):
    from padertorch_amd import _lib
    lib = _lib.load()
    if not lib.ptmi_lstm_split_enabled():
        pytest.skip('split recurrence kernels not active')
    buf = _Buffers(lib)
    ptrs = ('gates', 'c', 'c0', 'dhy', 'dc_n', 'w_t', 'dg', 'planes', 'bs', 'offs', 'masks', 'scratch', 'carry')

    def call(meta='equal', **over):
        m = buf.metas[meta]
        a = dict(gates=buf.gates, c=buf.c, c0=None, dhy=buf.dhy, dc_n=None, w_t=buf.w_t, dg=buf.dg, planes=None, bs=m.bs_dev,
                 offs=m.offs_dev, masks=None, scratch=buf.scratch[1], carry=None, T=T, B=m.max_batch, rows=m.rows, H=H, ndir=NDIR,
                 s_begin=0, s_end=T, prefilled=0)
        a.update(over)
        p = [a[k] if isinstance(a[k], int) else _lib.ptr(a[k]) for k in ptrs]
        return lib.ptmi_lstm_backward_persistent(*p, a['T'], a['B'], a['rows'], a['H'], a['ndir'], a['s_begin'], a['s_end'], a['prefilled'],
                                                 _lib.stream(torch.device(DEV)))

    cases = [(f'{k} is null', {k: None}, INVALID) for k in ('gates', 'c', 'dhy', 'w_t', 'bs', 'offs', 'scratch')]
    cases += [(f'{k} = {v}', {k: v}, INVALID) for k, v in (('T', 0), ('B', 0), ('H', 0), ('rows', 0), ('ndir', 0), ('ndir', 3))]
    cases += [
        ('dgates and dgates_t both null', dict(dg=None), INVALID),
        ('dgates_t not 16-byte aligned', dict(planes=buf.planes.data_ptr() + 2), INVALID),
        ('s_begin < 0', dict(s_begin=-1, carry=buf.carry), INVALID),
        ('s_end > T', dict(s_end=T + 1, carry=buf.carry), INVALID),
        ('s_begin >= s_end', dict(s_begin=2, s_end=2, carry=buf.carry), INVALID),
        ('a partial range without dc_carry', dict(s_end=T - 1), INVALID),
        ('dc_n with a partial range', dict(s_begin=1, carry=buf.carry, dc_n=buf.dc_n), INVALID),
        ('dc_n with step_masks', dict(dc_n=buf.dc_n, masks=buf.masks, carry=buf.carry), UNSUPPORTED),
        ('step_masks with c0', dict(masks=buf.masks, c0=buf.c0), UNSUPPORTED),
        ('step_masks with rows != T * max_batch', dict(masks=buf.masks, meta='ragged'), UNSUPPORTED),
        ('step_masks with max_batch > 64', dict(masks=buf.masks, meta='b80'), UNSUPPORTED),
        ('step_masks with a partial range', dict(masks=buf.masks, s_end=T - 1, carry=buf.carry), UNSUPPORTED),
        ('dgates_t for a ragged batch', dict(planes=buf.planes, meta='ragged'), UNSUPPORTED),
        ('dgates_t for a batch that is no multiple of 16', dict(planes=buf.planes, meta='b24'), UNSUPPORTED),
        ('H % 4 != 0', dict(H=6), UNSUPPORTED),
        ('a plan that is not supported', dict(f32=True), UNSUPPORTED),
    ]
    _run(lib, buf, call, cases, monkeypatch)


def test_forward_refusals(monkeypatch):
    from padertorch_amd import _lib
    lib = _lib.load()
    if not lib.ptmi_lstm_split_enabled():
        pytest.skip('split recurrence kernels not active')
    buf = _Buffers(lib)
    ptrs = ('gates', 'hy', 'c', 'c0', 'w_pad', 'w_amax', 'bs', 'offs', 'masks', 'scratch')

    def call(meta='equal', **over):
        m = buf.metas[meta]
        a = dict(gates=buf.gates.clone(), hy=buf.hy, c=buf.c, c0=None, w_pad=buf.w_pad, w_amax=None, bs=m.bs_dev, offs=m.offs_dev,
                 masks=None, scratch=buf.scratch[0], T=T, B=m.max_batch, rows=m.rows, H=H, KP=16, ndir=NDIR, prefilled=0,
                 backward_scratch=buf.scratch[1])
        a.update(over)
        p = [_lib.ptr(a[k]) for k in ptrs]
        return lib.ptmi_lstm_forward_persistent(*p, a['T'], a['B'], a['rows'], a['H'], a['KP'], a['ndir'], a['prefilled'],
                                                _lib.ptr(a['backward_scratch']), _lib.stream(torch.device(DEV)))

    cases = [(f'{k} is null', {k: None}, INVALID) for k in ('gates', 'hy', 'c', 'w_pad', 'bs', 'offs', 'scratch')]
    cases += [(f'{k} = {v}', {k: v}, INVALID) for k, v in (('T', 0), ('B', 0), ('H', 0), ('rows', 0), ('ndir', 0), ('ndir', 3))]
    cases += [
        ('step_masks with c0', dict(masks=buf.masks, c0=buf.c0), UNSUPPORTED),
        ('step_masks with rows != T * max_batch', dict(masks=buf.masks, meta='ragged'), UNSUPPORTED),
        ('step_masks with max_batch > 64', dict(masks=buf.masks, meta='b80'), UNSUPPORTED),
        ('H % 4 != 0', dict(H=6), UNSUPPORTED),
        ('KP is not H rounded up to 16', dict(KP=KP_MAX), UNSUPPORTED),
        ('a plan that is not supported', dict(f32=True), UNSUPPORTED),
    ]
    _run(lib, buf, call, cases, monkeypatch)
