"""The per-frame spectral gate (``oracle/stft_fp32.py``) on the host: what it passes, what it catches, and that the whole-tensor
gate of ``tests/test_gpu_stft.py`` (``atol = 2e-4 * max|ref|``) cannot see the same faults.  CPU only, oracle only.

Case: blackman, fading 'full', pad, B = 3, N = 6 * size + 17 (odd), ``RandomState(0).standard_normal`` - the last frame of a row then
holds 1 (size 64) / 17 (size 512) samples under the window's first taps and is 1.5e-18 / 4.1e-4 of the tensor's maximum.
Mutations (each of the fp64 oracle's own input or output, so that nothing but the mutation differs):
  * ``drop``  - the row's last valid sample reads as zero (a wrong patch of an odd-length row's last sample);
  * ``shift`` - the fading pad is one sample short (every sample lands one tap early);
  * ``scale`` - the last frame times 1.5.
``drop`` and ``shift`` come twice: on the whole input, and confined to the LAST frame - the frame whose samples the kernels fetch
through clamped addresses and selects, i.e. what a fault in that path alone would look like.
"""
import numpy as np
import pytest

from oracle import stft_np
from oracle import stft_fp32 as G

CASES = [(64, 16), (512, 128)]
#: the old gate's verdict on the last-frame mutations where the figures above decide it: at size 64 anything in the last frame is
#: invisible (1.5e-18 of the maximum); at size 512 ``drop`` errs by 1.5e-4 of the maximum (passes), ``scale`` by 2.06e-4 and ``shift``
#: by 7.3e-4 (on and beyond the edge of 2e-4: not asserted)
OLD_GATE_PASSES = {(64, 'drop_last'), (64, 'shift_last'), (64, 'scale'), (512, 'drop_last')}


def _case(size, shift):
    rng = np.random.RandomState(0)
    x = rng.standard_normal((3, 6 * size + 17)).astype(np.float32)
    want = stft_np.stft(x, size, shift)
    return x, want, G.stft32(x, size, shift)


def _mutations(x, want, size, shift):
    xd = x.copy()
    xd[:, -1] = 0.
    drop = stft_np.stft(xd, size, shift)
    xs = np.concatenate([x[:, 1:], np.zeros_like(x[:, :1])], axis=1)
    shifted = stft_np.stft(xs, size, shift)
    out = dict(drop=drop, shift=shifted)
    for name, full in (('drop_last', drop), ('shift_last', shifted)):
        out[name] = want.copy()
        out[name][:, -1] = full[:, -1]
    out['scale'] = want.copy()
    out['scale'][:, -1] *= 1.5
    return out


@pytest.mark.parametrize('size,shift', CASES + [(1024, 256), (100, 25)])
def test_fp32_restatement_passes_forward_and_inverse(size, shift):
    x, want, ref32 = _case(size, shift)
    assert ref32.dtype == np.complex64 and ref32.shape == want.shape
    assert G.check(ref32, want, ref32, f'restatement {size}/{shift}') == 1.
    r32 = G.frame_ratio(ref32, want).max()
    assert 1e-9 < r32 < 2e-7, r32            # fp32 arithmetic: a few 1e-8 of the frame's norm, on EVERY frame
    wi = stft_np.istft(want, size, shift)
    ri = G.istft32(want, size, shift)
    assert ri.dtype == np.float32 and ri.shape == wi.shape
    bw, br = G.blocks_of(wi, shift), G.blocks_of(ri, shift)
    assert bw.shape == (3, -(-wi.shape[-1] // shift), shift)
    G.check(br, bw, br, f'inverse restatement {size}/{shift}')
    assert 1e-9 < G.frame_ratio(br, bw).max() < 1e-6


@pytest.mark.parametrize('size,shift', CASES)
def test_mutations_fail_the_frame_gate_and_pass_the_tensor_gate(size, shift):
    x, want, ref32 = _case(size, shift)
    last = np.abs(want[:, -1]).max() / np.abs(want).max()
    print(f'size {size}: last frame max|X| / tensor max|X| = {last:.2e}')
    assert last < (1e-15 if size == 64 else 5e-4)
    for name, cand in _mutations(x, want, size, shift).items():
        r, r32 = G.gate_figures(cand, want, ref32)
        old = G.old_gate_passes(cand, want)
        print(f'size {size} {name}: max r / max r32 = {r / r32:.2e}, tensor gate error {np.abs(cand - want).max() / np.abs(want).max():.2e}'
              f' of max|ref| ({"passes" if old else "fails"})')
        assert r > 1e3 * G.MARGIN * r32, (name, r, r32)          # not a near miss: five to seven orders
        assert not G.passes(cand, want, ref32), name
        with pytest.raises(AssertionError):
            G.check(cand, want, ref32, name)
        if (size, name) in OLD_GATE_PASSES:
            assert old, (size, name)


def test_zero_frames_must_be_exactly_zero_and_finite():
    x, want, ref32 = _case(64, 16)
    want = np.concatenate([want, np.zeros_like(want[:, :2])], axis=1)      # frames past a ragged row's end
    ref32 = np.concatenate([ref32, np.zeros_like(ref32[:, :2])], axis=1)
    assert G.passes(ref32, want, ref32)
    bad = ref32.copy()
    bad[1, -1, 5] = 1e-30
    assert not G.passes(bad, want, ref32)
    with pytest.raises(AssertionError, match='exactly zero'):
        G.frame_ratio(bad, want)
    bad = ref32.copy()
    bad[0, 3, 0] = np.nan
    with pytest.raises(AssertionError, match='non-finite'):
        G.frame_ratio(bad, want)
    # the gate is per ROW and frame: an error of 1e-6 of one frame's norm in one bin of one row fails
    bad = ref32.astype(np.complex128)
    bad[2, 7, 11] += 1e-6 * np.linalg.norm(want[2, 7])
    assert not G.passes(bad, want, ref32) and G.old_gate_passes(bad, want)


def test_unsupported_logmel_request_names_lds_not_the_size():
    """``stft_logmel`` turns ``PTMI_E_UNSUPPORTED`` into this error: at a size that HAS a plan the reason is LDS."""
    from padertorch_amd.contrib.je.modules.features import _logmel_unsupported, _plan_lds_bytes
    # the launcher's own figures: 92 176 bytes at 2048 (what kept that plan from running under a 64 KiB limit), 40 976 at 512
    assert _plan_lds_bytes(2048) == 92176 and _plan_lds_bytes(1024) == 46096 and _plan_lds_bytes(512) == 40976
    for size in (64, 128, 256, 512, 1024, 2048):
        e = _logmel_unsupported(size, 80, 41600)             # a dense 80 x 513 bank: 166 400 bytes of weights alone
        assert isinstance(e, NotImplementedError) and 'LDS' in str(e) and 'power-of-two' not in str(e), str(e)
        assert '80 filters' in str(e) and f'size {size} ' in str(e)
        # a bank that DOES fit: the code then came from an index limit of the launcher, and the message must not blame LDS
        e = _logmel_unsupported(size, 80, 2000)
        assert isinstance(e, NotImplementedError) and 'LDS' not in str(e) and 'index range' in str(e), str(e)
    # exactly at the limit fits, one group of weights more does not
    room = (160 * 1024 - _plan_lds_bytes(2048) - 16 - 12 * 80) // 4
    assert 'LDS' not in str(_logmel_unsupported(2048, 80, room)) and 'LDS' in str(_logmel_unsupported(2048, 80, room + 8))
    e = _logmel_unsupported(400, 40, 2000)
    assert isinstance(e, NotImplementedError) and 'power-of-two' in str(e) and '(got 400)' in str(e) and 'LDS' not in str(e)
