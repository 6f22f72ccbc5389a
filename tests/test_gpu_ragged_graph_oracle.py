"""Replays of ONE captured ragged step (``data.StaticSlotBatcher`` -> ``train.graphed.GraphedStep``) against the fp64 oracle at each
batch's TRUE lengths.

``tests/test_gpu_ragged_graph.py`` holds replays against the eager loop on the same ``StaticSlots`` tables: a wrong table, or device
state one use leaves behind for the next (data-as-flag hand-off planes, arrival words, per-step row masks, idle grid rows after a longer
pattern), makes both paths wrong in the same way.  Here every replay is measured against ``oracle/torch_ref.py`` in fp64 (through
torch's native double kernels on the GPU, as ``tests/test_gpu_graphed_fullsize.py`` does) run from the parameters the replay started
from on the batch's examples cut to the frame counts of their sample counts:

  * the loss within 1e-4 x max(1, |loss|), every parameter's gradient - copied out of the flat bucket by a node of the graph in front
    of the clip + Adam kernel - within 2e-4 of its largest entry, the gradient norm within 5e-5;
  * the features the step starts from (waveforms -> STFT, device-side lengths) against ``torch_ref.features_from_waveforms`` on each
    example cut to its ``num_samples``.

The batches are all materialised before the first step, and the patterns come in an order in which every replay follows one that
leaves other state behind: a full grid, a short one (a long idle tail), one example at the padded maximum beside the shortest the
batcher takes (4 frames), an assignment of examples to slots that differs in every slot, the full grid again; and a layout with fewer
examples than slots (idle slots for the whole grid).  ``PTMI_GRAD_REPORT=<file>`` appends every replay's errors.
"""
import copy
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
LW = dict(pit_ips_loss=1., pit_mse_loss=0.)


def _utterances(rng, lengths, K):
    out = []
    for n in lengths:
        s = (0.1 * rng.standard_normal((K, int(n)))).astype(np.float32)
        out.append(dict(y=s.sum(0), s=s, num_samples=int(n)))
    return out


def _layout(batcher, num_samples):
    from padertorch_amd.ops.sequence import SlotLayout
    return SlotLayout(batcher.frames_of(num_samples), batcher.slots)


def _slot_members(lay):
    return [sorted((b, lay.t0[b]) for b in range(len(lay.lengths)) if lay.slot[b] == s) for s in range(lay.slots)]


def _patterns(case, rng, batcher):
    """Lengths (samples) of the batches of ``case``, in replay order, with the property each one is there for checked on the host."""
    E, S, T, n_max = batcher.examples, batcher.slots, batcher.steps, batcher.max_samples
    if case == 'order':
        full = [n_max] * E                                                         # (a) every slot full to the grid's capacity
        short = [int(v) for v in rng.randint(1800, 2900, E)]                       # (b) fewer than half the grid's steps
        tiny = [n_max] + [int(v) for v in rng.randint(1, 129, E - 1)]              # (c) the padded maximum + the shortest: 4 frames
        other = [int(v) for v in rng.randint(3200, n_max + 1, E)]                  # (d) another slot of every example
        lens = [full, short, tiny, other, full]                                    # (a') the full grid after (b) - (d)
        lays = [_layout(batcher, sorted(v, reverse=True)) for v in lens]
        assert lays[0].T == T and lays[1].T < T / 2 and lays[2].T == batcher.padded_time
        assert set(batcher.frames_of(tiny[1:])) == {4} and batcher.frames_of([129]) == [5]
        assert all(a != b for a, b in zip(_slot_members(lays[3]), _slot_members(lays[2])))
        return lens
    if case == 'idle slots':                                                       # fewer examples than slots
        return [[int(v) for v in rng.randint(n_max // 2, n_max + 1, E)] for _ in range(3)]
    return [[int(v) for v in rng.randint(n_max // 2, n_max + 1, E)] for _ in range(3)]      # the training distribution U[max / 2, max]


CASES = {
    # name: (kind, examples, slots, max samples, grid steps, model kwargs, pattern kind)
    'pit-8x4': ('pit', 8, 4, 6400, 106, dict(F=257, recurrent_layers=2, units=48, K=2), 'order'),
    'pit-4x8': ('pit', 4, 8, 6400, None, dict(F=257, recurrent_layers=2, units=48, K=2), 'idle slots'),
    'pit-64x32-blstm600': ('pit', 64, 32, 6 * 8000, None, dict(F=257, recurrent_layers=3, units=600, K=2), 'random'),
    'dc-8x4': ('dc', 8, 4, 6400, 106, dict(F=257, recurrent_layers=2, units=64, E=8, input_feature_transform='log1p'), 'order'),
}


def _features(kind, K):
    import padertorch_amd as pt
    from padertorch_amd.ops.sequence.pack_module import PaddedList

    def features(src):
        feats = pt.ops.pit_features(src['y'], src['s'], src['num_samples'], num_frames_dev=src['slots'].frames)
        if kind == 'pit':
            return dict(feats, slots=src['slots'])
        X = feats['X_abs'].padded
        target = torch.nn.functional.one_hot(X.argmax(2), K).permute(0, 1, 3, 2).to(torch.float32, memory_format=torch.contiguous_format)
        return dict(Y_abs=feats['Y_abs'], target_mask=PaddedList(target, feats['Y_abs'].lengths, True, feats['Y_abs'].lengths_dev),
                    slots=src['slots'])
    return features


def _check_features(feats, src, frames):
    """The eager features of one batch against ``torch_ref.features_from_waveforms`` in fp64 on each example cut to its sample count."""
    from oracle import torch_ref
    stft = torch_ref.ConvSTFT(512, 128)
    ns = src['num_samples'].tolist()
    y = [src['y'][b, :n].double() for b, n in enumerate(ns)]
    s = [src['s'][b, :, :n].double() for b, n in enumerate(ns)]
    ref = torch_ref.features_from_waveforms(stft, s, y)
    assert ref['num_frames'] == frames, (ref['num_frames'], frames)
    for b, t in enumerate(frames):
        for key in ('Y_abs', 'X_abs'):
            got = feats[key].padded[b]
            err = float((got[:t].double() - ref[key][b]).abs().max())
            assert err <= 2e-5, (key, b, err)
            if t < got.shape[0]:
                assert float(got[t:].abs().max()) == 0., (key, b)              # frames past the example's own count
        # cos(phase difference) is ill-conditioned where |Y| or |X| is ~0: weighted by magnitude (tests/test_gpu_stft.py)
        w = torch.minimum(ref['Y_abs'][b][:, None, :], ref['X_abs'][b])
        err = float(((feats['cos_phase_difference'].padded[b][:t].double() - ref['cos_phase_difference'][b]).abs() * w).max())
        assert err <= 2e-5, ('cos_phase_difference', b, err)


def _oracle_examples(kind, feats, frames):
    """The model input of the oracle: every example cut to its true frame count, sorted by descending length (``pack_sequence``)."""
    order = sorted(range(len(frames)), key=lambda b: -frames[b])
    if kind == 'pit':
        keys = ('Y_abs', 'X_abs', 'cos_phase_difference')
        return {k: [feats[k].padded[b, :frames[b]].detach() for b in order] for k in keys}
    return dict(Y_abs=[feats['Y_abs'].padded[b, :frames[b]].detach() for b in order],
                target_mask=[feats['target_mask'].padded[b, :frames[b]].detach() for b in order])


def _fp64(ref, state, batch, lw):
    """``oracle/torch_ref.py`` in fp64 from the parameters ``state`` -> (loss, {name: gradient}, gradient norm); on the GPU through
    torch's native double kernels (test infrastructure: nothing of the HIP library runs here)."""
    from oracle import torch_ref
    ref64 = copy.deepcopy(ref).double()
    ref64.load_state_dict({k: v.detach().cpu().double() for k, v in state.items()})
    ref64.to(DEV)
    b64 = {k: [t.double().to(DEV) for t in v] for k, v in batch.items()}
    loss = torch_ref.review_to_loss(ref64.review(b64, ref64(b64)), lw)
    loss.backward()
    grads = {k: q.grad.detach().cpu() for k, q in ref64.named_parameters()}
    norm = float(torch.sqrt(sum((g ** 2).sum() for g in grads.values())))
    return float(loss.detach()), grads, norm


@pytest.mark.parametrize('case', list(CASES))
def test_ragged_replays_vs_fp64_oracle(tmp_path, case):
    import padertorch_amd as pt
    from padertorch_amd.contrib.examples.source_separation.pit.model import PermutationInvariantTrainingModel
    from padertorch_amd.contrib.tcl.dc import DeepClusteringModel
    from padertorch_amd.data import StaticSlotBatcher, row_slot_batches
    from padertorch_amd.ops import lstm as _lstm
    from padertorch_amd.train.graphed import GraphedStep
    from oracle import torch_ref
    from test_gpu_graphed_fullsize import _restore
    kind, E, S, n_max, steps, model_kw, pattern = CASES[case]
    K = model_kw.get('K', 3)
    rng = np.random.RandomState(sum(map(ord, case)))
    batcher = StaticSlotBatcher(examples=E, slots=S, max_samples=n_max, device=DEV, steps=steps)
    lens = _patterns(pattern, rng, batcher)
    stream = _utterances(rng, [n for v in lens for n in v], K)
    data = [batcher(b) for b in row_slot_batches(stream, row_slots=S, fill=E / S)]        # all materialised before the first step
    assert batcher.refused == 0 and len(data) == len(lens)
    truth = [batcher.frames_of(d['num_samples'].tolist()) for d in data]
    for d, t in zip(data, truth):
        assert d['slots'].frames.tolist() == t

    torch.manual_seed(5)
    model = PermutationInvariantTrainingModel(**model_kw) if kind == 'pit' else DeepClusteringModel(**model_kw)
    ref = torch_ref.PITModelRef(**model_kw) if kind == 'pit' else torch_ref.DCModelRef(**model_kw)
    ref.load_state_dict(model.state_dict())
    lw = LW if kind == 'pit' else None
    tr = pt.Trainer(model, tmp_path, pt.optimizer.Adam(gradient_clipping=1.), loss_weights=lw, deferred_checks=True)
    tr.to(torch.device(DEV))
    tr._flat = tr.optimizer.use_flat_grads()
    tr.op_context.defer_wgrad = True
    _lstm.warm_side_stream(torch.device(DEV))
    model.train()
    init = {k: v.detach().clone() for k, v in model.state_dict().items()}
    features = _features(kind, K)

    # the eager features of every batch, against the oracle's from the waveforms, and cut to the true lengths for the oracle step
    inputs = []
    with torch.no_grad():
        for d, t in zip(data, truth):
            _check_features(pt.ops.pit_features(d['y'], d['s'], d['num_samples'], num_frames_dev=d['slots'].frames), d, t)
            feats = features(d)
            inputs.append({k: [x.cpu() for x in v] for k, v in _oracle_examples(kind, feats, t).items()})
            del feats

    # a node of the graph copies the step's gradients out of the bucket in front of the kernel that clips, applies and zeroes them
    snap = torch.zeros_like(tr._flat.flat)
    plain_step = tr.optimizer_step

    def optimizer_step_with_snapshot():
        _lstm.sync_deferred()
        snap.copy_(tr._flat.flat)
        return plain_step()
    tr.optimizer_step = optimizer_step_with_snapshot
    _lstm.CHECK_PERSISTENT_ERRORS = True
    try:
        step = GraphedStep(tr, [data[0]], prepare=features, warmup=1, clone_inputs=True)
        _restore(model, tr, init)
        losses, norms, started_from, grads = [], [], [], []
        for d in data:
            started_from.append({k: v.detach().clone() for k, v in model.state_dict().items()})
            step([d])
            sc = step.scalars()
            losses.append(sc['loss'])
            norms.append(sc['grad_norm'])
            grads.append(snap.clone())
        torch.cuda.synchronize()
        _lstm.check_errors()
    finally:
        _lstm.CHECK_PERSISTENT_ERRORS = False
    assert step.captures == 1
    names = [k for k, _ in model.named_parameters()]

    def by_name(flat):
        out, off = {}, 0
        for name, p in zip(names, tr._flat.params):
            out[name] = flat[off:off + p.numel()].view_as(p).detach().cpu().double()
            off += p.numel()
        return out

    failures = []
    for r, (batch, state) in enumerate(zip(inputs, started_from)):
        loss64, truth64, norm64 = _fp64(ref, state, batch, lw)
        got = by_name(grads[r])
        report = [(k, float((got[k] - q).abs().max()) / max(float(q.abs().max()), 1e-30)) for k, q in truth64.items()]
        if os.environ.get('PTMI_GRAD_REPORT'):
            with open(os.environ['PTMI_GRAD_REPORT'], 'a') as f:
                f.write(f'# ragged replay: {case} replay {r} frames {sum(truth[r])} in {S} x {data[r]["slots"].steps}: |loss - fp64| = '
                        f'{abs(losses[r] - loss64):.3e}, |grad norm - fp64| / fp64 = {abs(norms[r] - norm64) / norm64:.3e}, worst '
                        f'gradient {max(e for _, e in report):.3e} ({max(report, key=lambda x: x[1])[0]})\n')
                for k, e in report:
                    f.write(f'{k} hip {e:.3e}\n')
        if abs(losses[r] - loss64) > 1e-4 * max(1., abs(loss64)):
            failures.append(('loss', r, losses[r], loss64))
        failures += [('gradient', r, k, e) for k, e in report if e > 2e-4]
        if abs(norms[r] - norm64) > 5e-5 * norm64:
            failures.append(('grad norm', r, norms[r], norm64))
    assert not failures, failures
