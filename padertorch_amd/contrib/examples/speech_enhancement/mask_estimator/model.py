"""``SimpleMaskEstimator``: masked per-utterance normalisation -> BLSTM -> three dense layers -> sigmoid, trained
with binary cross-entropy on a speech and a noise mask.

Drop-in for ``padertorch/contrib/examples/speech_enhancement/mask_estimator/model.py:6-90``: the same
constructor arguments, the same ``forward(batch) -> dict`` / ``review(batch, output) -> dict`` contract and the
same ``state_dict`` (the layers sit in ``self.net`` at the reference's positions: ``net.0`` normalisation,
``net.1`` LSTM, ``net.3`` / ``net.6`` / ``net.8`` linears).  Differences: the normalisation and the LSTM run on the
HIP kernels (``modules.Normalization``, ``modules.StatefulLSTM``), and the summary images - a device -> host copy
each - are rendered only when ``create_snapshot`` is set (``base.py:300-306`` allows that) instead of on every
review.
"""
import torch
from torch.nn import functional as F

from ..... import base, modules
from .....ops import mappings
from .....summary import mask_to_image, stft_to_image

#: review keys of the images and where their data comes from: (dict, key, renderer)
_IMAGES = (
    ('speech_mask', 'output', 'speech_mask_prediction', mask_to_image),
    ('observed_stft', 'batch', 'observation_abs', stft_to_image),
    ('noise_mask', 'output', 'noise_mask_prediction', mask_to_image),
)


def _layers(num_features, num_units, dropout, activation):
    act = mappings.ACTIVATION_FN_MAP[activation]
    hidden = num_units // 4                 # per direction
    yield modules.Normalization('btf', (1, 1, num_features), statistics_axis='t', independent_axis='f',
                                batch_axis='b', sequence_axis='t')
    yield modules.StatefulLSTM(num_features, hidden, bidirectional=True, batch_first=True, save_states=False)
    for width_in in (2 * hidden, num_units):
        yield torch.nn.Dropout(dropout)
        yield torch.nn.Linear(width_in, num_units)
        yield act()
    yield torch.nn.Linear(num_units, 2 * num_features)      # speech mask | noise mask
    yield torch.nn.Sigmoid()


class SimpleMaskEstimator(base.Model):
    #: the vector ``enhance`` beamforms with: one of ``ops.beamforming.BEAMFORMERS`` (``'gev+ban'``: the neural-mask GEV beamformer
    #: with blind analytic normalization; ``gev*`` and ``pca*`` are phase-corrected along the bins and take no ``ref_channel``)
    beamformer: str = 'mvdr_souden'

    def __init__(self, num_features, num_units=1024, dropout=0.5, activation='elu'):
        super().__init__()
        self.num_features = num_features
        self.net = torch.nn.Sequential(*_layers(num_features, num_units, dropout, activation))

    def forward(self, batch):
        speech, noise = self.net(batch['observation_abs']).split(self.num_features, dim=-1)
        return dict(speech_mask_prediction=speech, noise_mask_prediction=noise)

    def review(self, batch, output):
        loss = sum(F.binary_cross_entropy(output[f'{k}_mask_prediction'], batch[f'{k}_mask_target'])
                   for k in ('noise', 'speech'))
        review = dict(loss=loss)
        if self.create_snapshot:
            review['images'] = self.add_images(batch, output)
        return review

    def enhance(self, y, num_samples=None, stft=None, ref_channel=None):
        """What the masks are trained for (the reference's ``evaluate.py:110-137``, there on the host): mixtures ``y [B, C, N]`` (or a
        list of ``[C, N_b]``) -> ``dict(masked=[...], beamformed=[...])``, per example one waveform ``[N_b]`` each: the first
        channel times its speech mask, and the mask-based beamformer ``self.beamformer`` (``ops.mask_beamforming``: channel medians
        of both masks; Souden MVDR by default, reference channel chosen on the device unless ``ref_channel`` names one).
        HIP STFT -> the model on the channels' magnitudes -> beamformer -> HIP iSTFT, cut to ``N_b``; nothing leaves the device in between.

        ``num_samples``: host integers, the valid samples of the rows of a padded ``[B, C, N]``.  The model's normalisation takes no
        lengths, so examples of ONE length go through as one batch and examples of differing lengths one by one, as in the
        reference's evaluation.  ``stft``: an ``ops.STFT`` with ``num_features`` bins (default ``STFT(1024, 256)``).  Runs in eval
        mode under ``torch.no_grad()``."""
        from .....ops import STFT
        from .....ops.beamforming import parse_beamformer
        stft = STFT(1024, 256) if stft is None else stft
        if stft.size // 2 + 1 != self.num_features or stft.complex_representation != 'complex':
            raise ValueError(f'enhance: a complex STFT with {self.num_features} bins, got size {stft.size} '
                             f'({stft.complex_representation})')
        parse_beamformer('enhance', self.beamformer, ref_channel)       # (before any kernel runs)
        examples = list(y.unbind(0)) if torch.is_tensor(y) else list(y)
        if not examples or any(e.dim() != 2 for e in examples):
            raise ValueError('enhance: mixtures [B, C, N] or a list of [C, N_b]')
        lengths = [e.shape[-1] for e in examples] if num_samples is None else [int(n) for n in num_samples]
        if len(lengths) != len(examples) or any(not 0 < n <= e.shape[-1] for n, e in zip(lengths, examples)):
            raise ValueError(f'enhance: one length in (0, N_b] per example, got {lengths}')
        training = self.training
        self.eval()
        try:
            with torch.no_grad():
                if len(set(lengths)) == 1 and len({e.shape[0] for e in examples}) == 1:
                    batch = y if torch.is_tensor(y) else torch.stack(examples)
                    masked, beamformed = self._enhance_batch(batch[..., :lengths[0]], stft, ref_channel)
                    return dict(masked=list(masked.unbind(0)), beamformed=list(beamformed.unbind(0)))
                pairs = [self._enhance_batch(e[None, :, :n], stft, ref_channel) for e, n in zip(examples, lengths)]
                return dict(masked=[m[0] for m, _ in pairs], beamformed=[b[0] for _, b in pairs])
        finally:
            self.train(training)

    def _enhance_batch(self, y, stft, ref_channel):
        """``y [B, C, N]`` -> ``(masked [B, N], beamformed [B, N])``."""
        from .....ops import mask_beamforming
        Y = stft(y)                                                       # [B, C, T, F] complex64
        B, C, T, F = Y.shape
        out = self(dict(observation_abs=Y.abs().reshape(B * C, T, F)))    # the channels are the model's batch
        speech = out['speech_mask_prediction'].reshape(B, C, T, F)
        noise = out['noise_mask_prediction'].reshape(B, C, T, F)
        spectra = torch.stack([speech[:, 0] * Y[:, 0], mask_beamforming(Y, speech, noise, ref_channel=ref_channel,
                                                                        beamformer=self.beamformer)])
        masked, beamformed = stft.inverse(spectra)[..., :y.shape[-1]]
        return masked, beamformed

    @staticmethod
    def add_images(batch, output):
        """First example of the (batch-first) tensors as tensorboard images (reference ``:74-90``); the target masks
        are added under the reference's condition (``'speech_mask_prediction' in batch``)."""
        src = dict(batch=batch or {}, output=output)
        images = {name: render(src[where][key], True) for name, where, key, render in _IMAGES if key in src[where]}
        if batch is not None and 'speech_mask_prediction' in batch:
            images['speech_mask_target'] = mask_to_image(batch['speech_mask_target'], True)
            if 'speech_mask_target' in batch:
                images['noise_mask_target'] = mask_to_image(batch['noise_mask_target'], True)
        return images
