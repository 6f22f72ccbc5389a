"""The d-vector speaker model of ``padertorch/contrib/tcl/speaker_embeddings/dvectors.py`` on this package's HIP path: ``ResNet34`` /
``ResNet18`` (https://doi.org/10.48550/arXiv.2007.02480) are a ``Conv2d``, a ``CNN2d`` with strided residual skips, a ``Conv2d``
(``csrc/je_conv2d.hip``), two ``reduce.Mean`` (``csrc/seq_pool.hip``) and a batch norm over the d-vectors (``ops.batch_norm_rows``);
``DVectorModel`` adds ``AngularPenaltySMLoss`` (``csrc/aam_softmax.hip``).  Constructor arguments and the attribute names
``input_convolution``, ``resnet``, ``output_convolution``, ``bn`` (an ``nn.BatchNorm1d(affine=False)`` that only holds the buffers) and
``loss.fc`` are the reference's: its ``state_dict`` loads with ``strict=True``.

    ResNet34 / ResNet18 .forward(x [B, T, F], seq_len) -> (dvectors [B, E], embeddings)
    DVectorModel.forward(example) -> the same, from example['features'] (a list of [T_b, F]) and example['num_frames']
    DVectorModel.review(example, outputs) -> {'loss', 'histograms': {'loss_'}, and in evaluation 'buffers': {'example_ids',
                                              'speaker_ids', 'dvectors' (unit norm)}}

No einops: ``b t f -> b 1 f t`` is a view that ``ops.je_conv2d.planes`` gathers once.

Not built: ``prepare_example`` (paderbox's host-side fbank: ``NotImplementedError``), ``modify_summary``'s EER / DCF (``eer_metrics.py``;
the base class's ``modify_summary`` refuses unconsumed buffers), the audio and image summary entries of ``review``, and the modules
``teacher_student.py`` and ``student_embeddings.py``.

The full-size configurations (256 channels with 3 x 3 kernels, the ``(2, 1)`` strided skips with ``normalize_skip_convs=True``,
``bias=False`` with ``norm='batch'`` and ``pre_activation=True``) are constructed as in the reference; a geometry beyond a bound of
``ops.je_conv2d`` (LDS halo, weight-gradient LDS) raises that module's ``NotImplementedError`` in the first forward - the convolution
kernels are not changed here.
"""
import inspect

import torch
from torch import nn

from .... import base
from ....ops.aam_softmax import batch_norm_rows
from ...je.modules.conv2d import CNN2d, Conv2d
from ...je.modules.reduce import Mean
from .loss import AngularPenaltySMLoss

__all__ = ['ResNet34', 'ResNet18', 'DVectorModel']


class _ResNet(base.Module):
    #: residual blocks per stage
    blocks = None
    #: the axis of the first (unmasked) mean over the output plane ``[B, E, F', T']``
    first_mean_axis = None

    def __init__(self, in_channels, channels, dvec_dim, activation_fn, norm, pre_activation):
        super().__init__()
        n = 2 * sum(self.blocks)
        out_channels = sum((2 * b * [c] for b, c in zip(self.blocks, channels)), [])
        assert len(out_channels) == n, len(out_channels)
        stage2, stage4 = 2 * self.blocks[0], 2 * sum(self.blocks[:3])
        stride = n * [(1, 1)]
        stride[stage2], stride[stage4] = (2, 2), (2, 1)
        residual_connections = n * [None]
        for i in range(0, n, 2):
            residual_connections[i] = i + 2
        self.embedding_dim = dvec_dim
        self.input_convolution = Conv2d(in_channels, channels[0], kernel_size=3, stride=2, bias=False, norm=norm)
        self.resnet = CNN2d(
            input_layer=False, output_layer=False, in_channels=channels[0], out_channels=out_channels, kernel_size=n * [3], stride=stride,
            pool_size=n * [1], pool_stride=n * [1], pool_type=n * [None], residual_connections=residual_connections,
            activation_fn=activation_fn, pre_activation=pre_activation, norm=norm, normalize_skip_convs=True)
        self.output_convolution = Conv2d(channels[-1], dvec_dim, kernel_size=3, stride=(2, 1), bias=False, activation_fn='relu', norm=norm,
                                         pre_activation=True)
        self.bn = nn.BatchNorm1d(self.embedding_dim, affine=False)

    def forward(self, x, seq_len):
        """``x [B, T, F]`` log-mel features, ``seq_len [B]`` frames before padding -> ``(dvectors [B, E], embeddings)``."""
        x = x[:, None].transpose(2, 3)                                  # 'b t f -> b 1 f t'
        x, seq_len = self.input_convolution(x, seq_len)
        x, seq_len = self.resnet(x, seq_len)
        x, seq_len = self.output_convolution(x, seq_len)
        embeddings = Mean(axis=self.first_mean_axis)(x)
        dvectors = Mean(axis=-1)(embeddings, seq_len)
        dvectors = dvectors.reshape(-1, self.embedding_dim)
        bn = self.bn
        dvectors = batch_norm_rows(dvectors, bn.running_mean, bn.running_var, bn.num_batches_tracked,
                                   training=bn.training or bn.running_mean is None, momentum=bn.momentum, eps=bn.eps)
        return dvectors, embeddings


class ResNet34(_ResNet):
    """ResNet34 for speaker embedding extraction: mean over the reduced frequency axis (``Mean(axis=-2)`` -> ``embeddings [B, E, T']``),
    then the masked mean over time, then the batch norm."""
    blocks = (3, 4, 6, 3)
    first_mean_axis = -2

    def __init__(self, in_channels=1, channels=(64, 128, 256, 256), dvec_dim=256, activation_fn='relu', norm='batch', pre_activation=True):
        super().__init__(in_channels, channels, dvec_dim, activation_fn, norm, pre_activation)


class ResNet18(_ResNet):
    """The ResNet18 configuration.  As written in the reference its first mean is ``Mean(axis=-1)`` - over TIME, unmasked - and the
    masked ``Mean(axis=-1)`` that follows then runs over the reduced FREQUENCY axis with the time lengths (``dvectors.py:167-169``):
    the other order than ``ResNet34``'s.  Reproduced word for word; ``embeddings`` is ``[B, E, F']`` here."""
    blocks = (2, 2, 2, 2)
    first_mean_axis = -1

    def __init__(self, in_channels=1, channels=(64, 128, 128, 256), dvec_dim=128, activation_fn='relu', norm='batch', pre_activation=True):
        super().__init__(in_channels, channels, dvec_dim, activation_fn, norm, pre_activation)


def _default(factory, name):
    return inspect.signature(factory).parameters[name].default


class DVectorModel(base.Model):
    """A d-vector extractor (``speaker_net``) and its classification loss (``loss``)."""

    def __init__(self, speaker_net: ResNet34, loss: AngularPenaltySMLoss, sampling_rate=16000):
        super().__init__()
        self.speaker_net = speaker_net
        self.sampling_rate = sampling_rate
        self.loss = loss

    @classmethod
    def finalize_dogmatic_config(cls, config):
        """The reference's defaults into a plain dict (there is no ``Configurable`` here): a ``ResNet34`` and an ``AngularPenaltySMLoss``
        whose ``in_features`` is the net's ``dvec_dim``; ``out_features`` (the number of speakers) has to be set by the caller."""
        net = config['speaker_net'] = {'factory': ResNet34, **config.get('speaker_net', {})}
        dvec_dim = net.get('dvec_dim', _default(net['factory'], 'dvec_dim'))
        config['loss'] = {'factory': AngularPenaltySMLoss, 'in_features': dvec_dim, **config.get('loss', {})}
        return config

    @classmethod
    def from_config(cls, config):
        config = cls.finalize_dogmatic_config({k: (dict(v) if isinstance(v, dict) else v) for k, v in config.items() if k != 'factory'})
        make = lambda node: node.pop('factory')(**node)         # noqa: E731
        return cls(**{k: make(dict(v)) if isinstance(v, dict) and 'factory' in v else v for k, v in config.items()})

    def prepare_example(self, example):
        raise NotImplementedError('DVectorModel.prepare_example: the host-side log-fbank features (paderbox) are not built')

    def forward(self, example):
        sequence = torch.nn.utils.rnn.pad_sequence(list(example['features']), batch_first=True)
        return self.speaker_net(sequence, example['num_frames'])

    def review(self, example, outputs):
        dvectors, embeddings = outputs
        loss = self.loss(dvectors, labels=example['speaker_id'])
        review = {'loss': loss, 'histograms': {'loss_': loss}}
        if not self.training:
            dvectors = dvectors / (torch.norm(dvectors, dim=1, keepdim=True) + 1e-8)
            review['buffers'] = {'example_ids': example['example_id'], 'speaker_ids': example['speaker_id'], 'dvectors': dvectors}
        return review
