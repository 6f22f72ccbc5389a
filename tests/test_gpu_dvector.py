"""``DVectorModel`` end to end on the GPU (``contrib/tcl/speaker_embeddings``): a tiny ``ResNet18``, 3 examples of 40 / 33 / 17 frames
with 16 features, 5 speakers.  The tail of the model - masked mean, batch norm, loss - is recomputed in fp64 from what it returns."""
import pytest
import torch
import torch.nn.functional as F

from test_gpu_aam_softmax import BN_GATES, GATES, rel, restatement

pytestmark = pytest.mark.gpu


def make(training):
    from padertorch_amd.contrib.tcl.speaker_embeddings import AngularPenaltySMLoss, DVectorModel, ResNet18
    torch.manual_seed(0)
    model = DVectorModel(ResNet18(channels=(4, 4, 8, 8), dvec_dim=8), AngularPenaltySMLoss(8, 5)).cuda().train(training)
    lens = [40, 33, 17]
    example = {'features': [torch.randn(n, 16).cuda() for n in lens], 'num_frames': lens, 'speaker_id': [4, 0, 4],
               'example_id': ['a', 'b', 'c']}
    return model, example


def test_training_step():
    model, example = make(True)
    weight = model.loss.fc.weight.detach().double().cpu()
    dvectors, embeddings = model(example)
    review = model.review(example, (dvectors, embeddings))
    review['loss'].backward()
    assert set(review) == {'loss', 'histograms'} and review['histograms']['loss_'] is review['loss']
    for name, p in model.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all(), name
    # ResNet18: the masked mean runs over the LAST axis of the returned embeddings with the time lengths behind the convolutions
    emb = embeddings.detach().double().cpu()
    lengths = torch.tensor(example['num_frames'])
    for conv in [model.speaker_net.input_convolution, *model.speaker_net.resnet.convs, model.speaker_net.output_convolution]:
        lengths = torch.as_tensor(conv.get_output_sequence_lengths(lengths.numpy()))
    mask = (torch.arange(emb.shape[-1])[None, :] < lengths[:, None]).double()[:, None, :]
    pooled = (emb * mask).sum(-1) / (mask.sum(-1) + 1e-6)
    assert rel(dvectors.detach(), F.batch_norm(pooled, None, None, training=True, eps=1e-5)) <= BN_GATES['y']
    want = restatement(dvectors.detach().double().cpu(), weight, torch.tensor(example['speaker_id']), 'aam', 30., 0.2)
    assert rel(review['loss'].detach(), want[0]) <= GATES['loss']
    assert rel(model.loss.fc.weight.detach(), want[3]) <= GATES['w_hat']
    assert int(model.speaker_net.bn.num_batches_tracked) == 1


def test_evaluation_fills_the_buffers():
    model, example = make(False)
    with torch.no_grad():
        review = model.review(example, model(example))
    assert review['buffers']['example_ids'] == ['a', 'b', 'c'] and review['buffers']['speaker_ids'] == [4, 0, 4]
    norms = review['buffers']['dvectors'].norm(dim=1)
    assert tuple(review['buffers']['dvectors'].shape) == (3, 8) and torch.allclose(norms, torch.ones_like(norms), atol=1e-6)
    assert torch.isfinite(review['loss'])
