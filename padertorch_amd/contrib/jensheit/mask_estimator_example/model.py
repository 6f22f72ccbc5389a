"""``MaskEstimatorModel`` of ``padertorch/contrib/jensheit/mask_estimator_example/model.py:30-255``: the ``Model`` (``forward`` /
``review``) that makes :class:`MaskEstimator` trainable.

Same constructor, ``finalize_dogmatic_config``, output keys, review keys (``MaskLossKeys``) and ``state_dict`` (``estimator.*``) as
the reference.  The loss bookkeeping is the reference's ``add_losses`` (``:128-237``): per example the binary cross-entropy on the
speech and the noise logits pooled by ``reduction``, SUMMED over the batch; ``mask_loss`` their sum (plus the reconstruction loss);
with ``observation_stft`` in the batch the same losses weighted by the observation's power.  Where the reference loops over the
examples (two unreduced loss tensors, a pooling and two weighted sums each, and a host -> device copy of the power weights), here one
``ops.mask_bce_loss`` call per mask takes the padded ``[B, C, T, F]`` logits the estimator wrote, the device lengths and the complex
STFT as they are (``csrc/mask_loss.hip``); backward is one kernel per mask.

The lists ``forward`` returns are :class:`MaskList` s: plain lists of ``[C, T_b, F]`` views for every caller of the reference's
contract, which also carry the padded storage and the device lengths.  ``review`` uses the storage while the list is ``intact()`` and
pads the entries it is given otherwise.

Deliberate differences from the reference:

* ``reduction='average'`` (the reference's default) names no entry of its pooling map (``:11-16``: median, mean, min, max), so the
  reference cannot run a review with its own default.  Here ``'average'`` is an alias of ``'mean'``; any other unknown name is a
  ``ValueError`` at construction.
* the reference leaves the VAD loss unreduced (``[C, T_b, 1]`` per example, ``:201-205``), which makes the total loss non-scalar and
  ragged batches unsummable.  With ``vad`` in the batch and ``vad_logits`` in the output ``review`` raises ``NotImplementedError``
  instead of inventing a reduction.
* ``audios`` (``transformer.inverse``: an ``ops.STFT``, on the device) and ``images`` are made only when ``create_snapshot`` is set,
  as ``SimpleMaskEstimator`` does and ``base.py`` allows.
"""
import numpy as np
import torch

from .... import _lib, base
from ....ops import losses
from ....ops.mask_loss import MASK_REDUCTIONS, mask_bce_loss
from ....ops.sequence import pad_sequence
from ....summary import mask_to_image, stft_to_image
from .modul import MaskEstimator
from .modul import MaskKeys as K

__all__ = ['MaskLossKeys', 'MaskEstimatorModel', 'MaskList', 'maybe_remove_channel']


class MaskLossKeys:
    NOISE_MASK = 'noise_mask_loss'
    SPEECH_MASK = 'speech_mask_loss'
    WEIGHTED_NOISE_MASK = 'power_weighted_noise_mask_loss'
    WEIGHTED_SPEECH_MASK = 'power_weighted_speech_mask_loss'
    MASK = 'mask_loss'
    WEIGHTED_MASK = 'power_weighted_mask_loss'
    TOTAL_MASK = 'total_mask_loss'
    VAD = 'VAD_loss'
    REC = 'reconstruction_loss'


class MaskList(list):
    """The per-example ``[C, T_b, ...]`` views into ONE padded ``[B, C, T, ...]`` tensor (``ops.sequence.PaddedList`` for the
    estimator's example-major, channel-second outputs).

    Attributes: ``padded``, ``lengths`` (host ints), ``lengths_dev`` (int32 device tensor ``[B]``)."""

    def __init__(self, padded, lengths, lengths_dev=None):
        lengths = [int(n) for n in lengths]
        super().__init__(v[:, :n] for v, n in zip(padded.unbind(0), lengths))
        self.padded = padded
        self.lengths = lengths
        self.lengths_dev = _lib.host_to_device(lengths, torch.int32, padded.device) if lengths_dev is None else lengths_dev

    def intact(self):
        """Are the entries still the views into ``padded`` the list was built with (``PaddedList.intact``)?  A caller may replace, drop
        or re-order entries; ``review`` asks first and pads the entries otherwise."""
        pad = self.padded
        if len(self) != len(self.lengths):
            return False
        step, base_ptr, inner = pad.stride(0) * pad.element_size(), pad.data_ptr(), pad.stride()[1:]
        return all(torch.is_tensor(v) and v.dim() == pad.dim() - 1 and v.data_ptr() == base_ptr + b * step and v.shape[1] == n
                   and v.shape[0] == pad.shape[1] and v.stride() == inner
                   for b, (v, n) in enumerate(zip(self, self.lengths)))


def _pad_examples(examples):
    """List of ``[C, T_b, F]`` tensors -> ``([B, C, T, F]`` (a view of the one ``[B, T, C, F]`` buffer a single padding call fills``),
    lengths)``."""
    lengths = [int(e.shape[1]) for e in examples]
    padded = pad_sequence([e.transpose(0, 1) for e in examples], batch_first=True)
    return padded.permute(0, 2, 1, 3), lengths


def _padded(name, value, device=None, dtype=None):
    """A batch entry or an output of ``forward`` -> ``(padded [B, C, T, F], lengths or None, lengths_dev or None)``: a
    :class:`MaskList` still intact gives its storage; any other list is padded (numpy entries on the host, then moved once); a tensor
    or array is taken as the padded batch."""
    if isinstance(value, MaskList) and value.intact():
        return value.padded, value.lengths, value.lengths_dev
    if isinstance(value, (list, tuple)):
        if len(value) == 0:
            raise ValueError(f'MaskEstimatorModel.review: {name} is empty')
        if all(torch.is_tensor(v) for v in value):
            padded, lengths = _pad_examples(list(value))
            return padded, lengths, None
        arrays = [np.asarray(v) for v in value]
        lengths = [a.shape[1] for a in arrays]
        C, _, F = arrays[0].shape
        host = np.zeros((len(arrays), C, max(lengths), F), dtype=np.result_type(*arrays))
        for b, a in enumerate(arrays):
            host[b, :, :a.shape[1]] = a
        value = host
    else:
        lengths = None
    if isinstance(value, np.ndarray):
        if dtype is not None:
            value = value.astype(dtype, copy=False)
        value = torch.from_numpy(np.ascontiguousarray(value)).to(device, non_blocking=True)
    if not torch.is_tensor(value) or value.dim() != 4:
        raise ValueError(f'MaskEstimatorModel.review: {name} is a list of [C, T_b, F] or one padded [B, C, T, F], got '
                         f'{tuple(value.shape) if hasattr(value, "shape") else type(value)}')
    return value, lengths, None


class MaskEstimatorModel(base.Model):
    """The mask estimator of Heymann 2016 (https://groups.uni-paderborn.de/nt/pubs/2016/icassp_2016_heymann_paper.pdf) as a trainable
    model.

    ``reduction``: how an example's element losses are pooled: ``'mean'``, ``'median'`` (torch's lower median), ``'min'``, ``'max'``;
    ``'average'`` - the reference's default, which its own pooling map does not know - is an alias of ``'mean'``."""

    @classmethod
    def finalize_dogmatic_config(cls, config):
        config['estimator'] = dict(factory=MaskEstimator)
        return config

    @classmethod
    def from_defaults(cls, num_features=513, transformer=None, reduction='average', sample_rate=16000, **estimator_updates):
        """The model around ``MaskEstimator.from_defaults(num_features, **estimator_updates)``."""
        return cls(MaskEstimator.from_defaults(num_features=num_features, **estimator_updates), transformer=transformer,
                   reduction=reduction, sample_rate=sample_rate)

    def __init__(self, estimator, transformer=None, reduction: str = 'average', sample_rate: int = 16000):
        super().__init__()
        if reduction != 'average' and reduction not in MASK_REDUCTIONS:
            raise ValueError(f"MaskEstimatorModel: reduction one of {sorted(MASK_REDUCTIONS)} (or 'average', an alias of 'mean'), "
                             f'got {reduction!r}')
        self.estimator = estimator
        self.transformer = transformer
        self.reduction = reduction
        self.sample_rate = sample_rate

    @property
    def pooling(self):
        """The name ``ops.mask_bce_loss`` is called with."""
        return 'mean' if self.reduction == 'average' else self.reduction

    def forward(self, batch):
        """``batch``: dict of lists; ``observation_abs`` a list of ``[C, T_b, F]`` (frames descending), ``num_frames`` their lengths.
        Returns per output key a :class:`MaskList` of ``[C, T_b, F]`` views cut to ``num_frames``."""
        obs = batch[K.OBSERVATION_ABS]
        num_frames = [int(n) for n in batch[K.NUM_FRAMES]]
        out = self.estimator(obs, num_frames)
        assert isinstance(out, dict)
        lengths_dev = None
        result = {}
        for key, value in out.items():
            result[key] = entry = MaskList(value, num_frames, lengths_dev)
            lengths_dev = entry.lengths_dev            # one copy of the lengths for all keys
        return result

    def review(self, batch, output):
        losses_ = self.add_losses(batch, output)
        review = dict(loss=losses_.pop(MaskLossKeys.MASK), scalars=losses_)
        if self.create_snapshot:
            review['audios'] = self.add_audios(batch, output)
            review['images'] = self.add_images(batch, output)
        return review

    def add_images(self, batch, output):
        images = dict()
        if K.SPEECH_PRED in output:
            images['speech_pred'] = mask_to_image(output[K.SPEECH_PRED][0], True)
        if K.SPEECH_MASK_PRED in output:
            images['speech_mask'] = mask_to_image(output[K.SPEECH_MASK_PRED][0], True)
        images['observed_stft'] = stft_to_image(batch[K.OBSERVATION_ABS][0], True)
        if K.NOISE_MASK_PRED in output:
            images['noise_mask'] = mask_to_image(output[K.NOISE_MASK_PRED][0], True)
        if batch is not None and K.SPEECH_MASK_TARGET in batch:
            images['speech_mask_target'] = mask_to_image(batch[K.SPEECH_MASK_TARGET][0], True)
            if K.NOISE_MASK_TARGET in batch:
                images['noise_mask_target'] = mask_to_image(batch[K.NOISE_MASK_TARGET][0], True)
        return images

    def add_audios(self, batch, output):
        audio_dict = dict()
        if K.OBSERVATION in batch:
            audio_dict[K.OBSERVATION] = (maybe_remove_channel(batch[K.OBSERVATION][0]), self.sample_rate)
        if K.SPEECH_IMAGE in batch:
            audio_dict[K.SPEECH_IMAGE] = (maybe_remove_channel(batch[K.SPEECH_IMAGE][0]), self.sample_rate)
        if self.transformer is None or K.OBSERVATION_STFT not in batch:
            return audio_dict
        with torch.no_grad():
            for key in (K.SPEECH_PRED, K.SPEECH_MASK_PRED):
                if key not in output:
                    continue
                pred = output[key][0].detach()
                obs = torch.as_tensor(batch[K.OBSERVATION_STFT][0]).to(pred.device).to(torch.complex64)[:, :pred.shape[1]]
                if key == K.SPEECH_PRED:                                 # the prediction's magnitude on the observation's phase
                    obs = torch.polar(torch.ones_like(pred), torch.angle(obs))
                audio_dict[key] = (maybe_remove_channel(self.transformer.inverse(pred * obs)), self.sample_rate)
        return audio_dict

    def _mask_loss(self, name, logits, target, power):
        """One mask of the whole batch: ``(sum_b pooled, sum_b weighted or None)``."""
        x, lengths, lengths_dev = _padded(name + ' logits', logits)
        T = x.shape[2]
        t, t_lengths, _ = _padded(name + ' target', target, x.device, np.float32)
        if lengths is None:
            lengths = t_lengths
        if t_lengths is not None and lengths is not None and list(t_lengths) != list(lengths):
            raise ValueError(f'MaskEstimatorModel.review: {name} target frames {t_lengths}, logits frames {lengths}')
        if t.shape[2] > T:
            t = t[:, :, :T]
        if lengths_dev is None and lengths is not None:
            lengths_dev = lengths
        pooled, weighted = mask_bce_loss(x, t.to(x.device), lengths_dev, None if power is None else power[:, :, :T], self.pooling)
        return pooled.sum(), (None if weighted is None else weighted.sum())

    def add_losses(self, batch, output):
        if K.VAD in batch and K.VAD_LOGITS in output:
            raise NotImplementedError(
                'MaskEstimatorModel.review: the reference leaves the VAD loss unreduced ([C, T_b, 1] per example), which makes the '
                'total loss non-scalar and a ragged batch unsummable; no reduction is invented here - drop vad from the batch')
        loss, weighted_loss, result = [], [], dict()
        if K.SPEECH_TARGET in batch and K.SPEECH_PRED in output:
            # (F.mse_loss: the mean over all elements; pooling a scalar leaves it as it is)
            rec = sum(losses.mse_loss(pred.reshape(1, -1), torch.as_tensor(target).to(pred.device).reshape(1, -1))
                      for target, pred in zip(batch[K.SPEECH_TARGET], output[K.SPEECH_PRED]))
            loss.append(rec)
            result[MaskLossKeys.REC] = rec
        power = None
        pairs = [(MaskLossKeys.NOISE_MASK, 'noise', K.NOISE_MASK_TARGET, K.NOISE_MASK_LOGITS),
                 (MaskLossKeys.SPEECH_MASK, 'speech', K.SPEECH_MASK_TARGET, K.SPEECH_MASK_LOGITS)]
        for loss_key, name, target_key, logits_key in pairs:
            if target_key not in batch or logits_key not in output:
                continue
            if K.OBSERVATION_STFT in batch and power is None:           # once for both masks
                device = output[logits_key][0].device
                power, _, _ = _padded('observation_stft', batch[K.OBSERVATION_STFT], device, np.complex64)
                power = power.to(device)
                if power.is_complex() and power.dtype != torch.complex64:
                    power = power.to(torch.complex64)
            pooled, weighted = self._mask_loss(name, output[logits_key], batch[target_key], power)
            loss.append(pooled)
            result[loss_key] = pooled
            if weighted is not None:
                weighted_loss.append(weighted)
        if loss:
            if K.OBSERVATION_STFT in batch:
                result[MaskLossKeys.WEIGHTED_MASK] = sum(weighted_loss)
            result[MaskLossKeys.MASK] = sum(loss)
        return result


def maybe_remove_channel(signal, exp_dim=1, ref_channel=0):
    if isinstance(signal, torch.Tensor):
        dim = signal.dim()
    elif isinstance(signal, np.ndarray):
        dim = signal.ndim
    else:
        raise ValueError
    if dim == exp_dim + 1:
        assert signal.shape[0] < 20, f'The first dim is supposed to be the ' \
            f'channel dimension, however the shape is {signal.shape}'
        return signal[ref_channel]
    elif dim == exp_dim:
        return signal
    else:
        raise ValueError(f'Either the signal has ndim {exp_dim} or'
                         f' {exp_dim +1}', signal.shape)
