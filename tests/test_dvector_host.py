"""The d-vector model's host side (``contrib/tcl/speaker_embeddings``): constructors, configuration, state_dict names, refusals.  No GPU."""
import pytest
import torch

from padertorch_amd.contrib.tcl.speaker_embeddings import AngularPenaltySMLoss, DVectorModel, ResNet18, ResNet34
from padertorch_amd.ops import aam_softmax


@pytest.mark.parametrize('loss_type,s,m', [('aam', 30.0, 0.2), ('arcface', 64.0, 0.5), ('sphereface', 64.0, 1.35)])
def test_loss_defaults_per_type(loss_type, s, m):
    loss = AngularPenaltySMLoss(8, 5, loss_type=loss_type.upper())
    assert (loss.loss_type, loss.s, loss.m, loss.eps, loss.reduce) == (loss_type, s, m, 1e-7, 'mean')
    assert tuple(loss.fc.weight.shape) == (5, 8) and loss.fc.bias is None
    assert (AngularPenaltySMLoss(8, 5, loss_type, s=10., m=0.1).s, AngularPenaltySMLoss(8, 5, loss_type, s=10., m=0.1).m) == (10., 0.1)


def test_finalize_dogmatic_config_wires_in_features():
    config = DVectorModel.finalize_dogmatic_config({})
    assert config['speaker_net']['factory'] is ResNet34 and config['loss']['in_features'] == 256
    config = DVectorModel.finalize_dogmatic_config({'speaker_net': {'factory': ResNet18, 'dvec_dim': 8}, 'loss': {'out_features': 5}})
    assert config['loss'] == {'factory': AngularPenaltySMLoss, 'in_features': 8, 'out_features': 5}
    model = DVectorModel.from_config({'speaker_net': {'factory': ResNet18, 'channels': (4, 4, 8, 8), 'dvec_dim': 8},
                                      'loss': {'out_features': 5}})
    assert tuple(model.loss.fc.weight.shape) == (5, 8) and model.sampling_rate == 16000
    with pytest.raises(NotImplementedError):
        model.prepare_example({})


# a skip convolution exists where the channels change: with (4, 4, 8, 8) that is the third stage, with (4, 8, 8, 16) the strided ones
@pytest.mark.parametrize('net,channels,skip', [(ResNet18, (4, 4, 8, 8), '8->10'), (ResNet34, (4, 4, 8, 8), '14->16'),
                                               (ResNet18, (4, 8, 8, 16), '4->6'), (ResNet34, (4, 8, 8, 16), '26->28')])
def test_state_dict_has_the_reference_names(net, channels, skip):
    model = DVectorModel(net(channels=channels, dvec_dim=8), AngularPenaltySMLoss(8, 5))
    names = set(model.state_dict())
    for name in ('input_convolution.conv.weight', 'resnet.convs.0.conv.weight', f'resnet.residual_skip_convs.{skip}.conv.weight',
                 'output_convolution.norm.gamma', 'bn.running_mean'):
        assert 'speaker_net.' + name in names, name
    assert 'loss.fc.weight' in names
    assert not [n for n in names if 'put_convolution' in n and n.endswith('bias')]     # bias=False on the input / output convolution
    assert len(model.speaker_net.resnet.convs) == {ResNet18: 16, ResNet34: 32}[net]


def test_refusals():
    e, w, y = torch.zeros(3, 8), torch.ones(5, 8), torch.tensor([0, 1, 2])
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        aam_softmax.angular_softmax_loss(e, w, y)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        aam_softmax.batch_norm_rows(e, None, None, None, True, 0.1, 1e-5)
    E = aam_softmax.max_features() + 1
    with pytest.raises(NotImplementedError, match='ptmi_aam_max_features'):
        aam_softmax.angular_softmax_loss(torch.zeros(3, E), torch.ones(5, E), y)
    from padertorch_amd import _lib
    lib = _lib.load()
    assert (lib.ptmi_aam_class_tile(), lib.ptmi_aam_row_tile(), lib.ptmi_aam_max_features()) == (aam_softmax.kAamBN, aam_softmax.kAamBM, 512)
