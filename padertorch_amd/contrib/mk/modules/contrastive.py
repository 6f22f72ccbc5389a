"""Contrastive predictive coding on 1-d data (``padertorch/contrib/mk/modules/contrastive.py``): ``CPC1d`` and ``CPCFeatureExtractor``
with the reference's constructor arguments, attribute names (a reference ``state_dict`` loads strictly), ``encode``, ``predict``,
``contrast``, ``forward``, ``review``, ``get_posteriors``, ``modify_summary`` and review keys; encoder and projection heads are the
``CNN1d`` / ``CNNTranspose1d`` / hybrid CNN of ``contrib/je`` on their HIP kernels, ``l2_normalization`` is ``modules.normalization.normalize``.

The hot path - ``contrast`` plus the cross-entropy, ``argmax`` and ``> -inf`` count of ``review`` - is ``ops.cpc_contrast.contrastive_scores``
(``csrc/cpc_contrast.hip``): the reference's dense logits ``[b, K, T_s]`` per step are never written.

Departures from the reference:

* ``outputs[0]`` of ``forward`` is the list of ``ContrastStats(ce, hits, finite, logits)`` per prediction step, not dense logits;
  ``review`` and ``get_posteriors`` (``exp(-ce)``) read the statistics, ``negatives`` is ``mean(finite - 1)``.
* the extra keyword ``dense_logits=False``: with ``True`` ``.logits`` holds the reference's tensor (stored by the same forward launch).
* ``contrast()`` returns ``(stats, targets)``.
* ``similarity='cosine'`` raises ``NotImplementedError`` (its clamp couples both norms inside the score).
* feature size ``d <= 512`` and, with ``negatives_mode='batch'``, ``b <= 64``: ``NotImplementedError`` beyond.
"""
import typing as tp

import numpy as np
import torch

from .... import base as pt_base
from ....contrib.je.modules.conv import CNN1d
from ....contrib.je.modules.conv_transpose import CNNTranspose1d
from ....contrib.je.modules.reduce import Mean
from ....modules.normalization import normalize
from ....ops.cpc_contrast import contrastive_scores

__all__ = ['CPC1d', 'CPCFeatureExtractor', 'repeat_interleaved', 'interleave', 'cosine_similarity', 'SIMILARITIES']


def repeat_interleaved(x, n):
    """``[x0, x0, .., x1, x1, ..]`` along the first axis (``n`` copies of each entry)."""
    return x.unsqueeze(1).repeat((1, n) + (x.dim() - 1) * (1,)).reshape(x.shape[0] * n, *x.shape[1:])


def interleave(x, y, dim):
    """``x`` and ``y`` alternating along ``dim``."""
    assert len(x.shape) > dim >= 0, dim
    shape = [*x.shape]
    shape[dim] *= 2
    return torch.stack((x, y), dim=dim + 1).view(shape)


def cosine_similarity(tensor, other, eps=1e-12):
    """``tensor (..., b, d) @ other (..., d, b)`` over the product of the norms, clamped at ``eps`` (a helper; not a ``CPC1d`` similarity here)."""
    prod = torch.matmul(tensor, other)
    norm = torch.linalg.norm(tensor, ord=None, dim=-1, keepdim=True) * torch.linalg.norm(other, ord=None, dim=-2, keepdim=True)
    return prod / torch.maximum(norm, torch.tensor(eps).to(norm.device))


SIMILARITIES = dict(dot_product=torch.matmul, cosine=cosine_similarity)


class CPC1d(pt_base.Model):
    """Contrastive Predictive Coding (van den Oord et al., 2018); arguments as the reference's ``CPC1d`` plus ``dense_logits``."""

    def __init__(self, encoder, fwd_projection_head, bwd_projection_head, feature_extractor, *, fwd_prediction_steps,
                 bwd_prediction_steps, multi_view=False, second_view_extractor=None, temperature=1., l2_normalization=False,
                 negatives_mode='batch', negative_to_target_dist=0, input_key='x', input_seq_len_key='seq_len_x', prefix=None,
                 similarity='dot_product', batch_mask_key: tp.Optional[str] = None, time_mask_key: tp.Optional[str] = None,
                 invert_batch_mask: bool = False, negative_ratio: float = 1., dense_logits: bool = False):
        super().__init__()
        self.feature_extractor = feature_extractor
        self.encoder = encoder
        assert len(fwd_prediction_steps) > 0
        assert all([s >= 0 for s in fwd_prediction_steps])
        if bwd_prediction_steps:
            assert all([s <= 0 for s in bwd_prediction_steps])
            assert not ((fwd_projection_head is None) ^ (bwd_projection_head is None))
        if similarity not in SIMILARITIES:
            raise KeyError(similarity)
        if similarity != 'dot_product':
            raise NotImplementedError(f'CPC1d: similarity={similarity!r}; the fused contrast kernel computes dot products only')
        self.fwd_projection_head = fwd_projection_head
        self.bwd_projection_head = bwd_projection_head
        self.fwd_prediction_steps = sorted(fwd_prediction_steps)
        self.bwd_prediction_steps = sorted(bwd_prediction_steps) if bwd_prediction_steps else []
        self.multi_view = multi_view
        self.second_view_extractor = second_view_extractor
        self.temperature = temperature
        self.l2_normalization = l2_normalization
        self.negatives_mode = negatives_mode
        self.negative_to_target_dist = negative_to_target_dist
        self.input_key = input_key
        self.input_seq_len_key = input_seq_len_key
        self.prefix = "" if prefix is None else prefix + "_"
        self.similarity = SIMILARITIES[similarity]
        self.batch_mask_key = batch_mask_key
        self.time_mask_key = time_mask_key
        self.invert_batch_mask = invert_batch_mask
        self.negative_ratio = negative_ratio
        self.dense_logits = dense_logits

    @property
    def prediction_steps(self):
        return self.bwd_prediction_steps + self.fwd_prediction_steps

    @staticmethod
    def _merge_features(x):
        return x.reshape(x.shape[0], x.shape[1] * x.shape[2], x.shape[3])          # 'b d f t -> b (d f) t'

    def encode(self, x, seq_len_x, target_shape=None):
        if self.multi_view:
            if self.second_view_extractor is not None:
                x_targets, seq_len_targets = self.second_view_extractor(x, seq_len=seq_len_x)
            elif self.feature_extractor is not None:
                x_targets, seq_len_targets = self.feature_extractor(x, seq_len=seq_len_x)
            else:
                raise ValueError('multi_view training requires two different views, i.e. two separate feature_extractors or one '
                                 'feature_extractor with data augmentation.')
        else:
            x_targets = seq_len_targets = None
        if self.feature_extractor is not None:
            x, seq_len_x = self.feature_extractor(x, seq_len=seq_len_x)
        if x_targets is not None:
            x = torch.cat((x, x_targets), dim=0)
            assert (np.array(seq_len_x) == seq_len_targets).all()
            seq_len_x = np.concatenate((seq_len_x, seq_len_targets))
        if isinstance(self.encoder, (CNN1d, CNNTranspose1d)) and x.dim() != 3:
            assert x.dim() == 4, x.dim()
            x = self._merge_features(x)
        if isinstance(self.encoder, CNNTranspose1d):
            if target_shape is not None:
                target_shape = list(target_shape)
                target_shape[1] = self.encoder.out_channels[-1]
            kwargs = dict(target_shape=target_shape)
        else:
            kwargs = {}
        if self.encoder is None:
            z, seq_len_z = x, seq_len_x
        else:
            z, seq_len_z = self.encoder(x, seq_len_x, **kwargs)
        if z.dim() == 4:
            z = self._merge_features(z)
        return x, z, seq_len_z

    def predict(self, z, seq_len_z):
        if self.fwd_projection_head is None:
            z_hat = z.repeat(1, len(self.fwd_prediction_steps), 1)
        else:
            z_hat, _ = self.fwd_projection_head(z, seq_len_z)
        if self.bwd_prediction_steps:
            if self.bwd_projection_head is None:
                z_hat_bwd = z.repeat(1, len(self.bwd_prediction_steps), 1)
            else:
                z_hat_bwd, _ = self.bwd_projection_head(z, seq_len_z)
            z_hat = torch.cat((z_hat_bwd, z_hat), dim=1)
        return z_hat

    def _log_batch_mask(self, batch_labels, b, device):
        """contrastive.py:350-368, on the host: ``[b, b]`` of 0 / -inf."""
        if batch_labels is None:
            return None
        if torch.is_tensor(batch_labels):
            batch_labels = batch_labels.detach().cpu().numpy()
        batch_labels = np.asarray(batch_labels)
        batch_mask = batch_labels[:, None] != batch_labels[None, :]
        if self.invert_batch_mask:
            batch_mask = (~batch_mask).astype(np.float32)                            # draw negatives with the same label
        else:
            batch_mask = batch_mask.astype(np.float32) + np.eye(b, dtype=np.float32)   # do not mask the same example
        with np.errstate(divide='ignore'):
            return torch.from_numpy(np.log(batch_mask)).to(device)

    def contrast(self, z_hat, z, batch_labels=None):
        s = len(self.prediction_steps)
        b, d, t = z.shape
        if self.l2_normalization:
            z, *_ = normalize(z, None, None, (1,), 0, 2, None, True, True, 1e-3)
            z_hat, *_ = normalize(z_hat.reshape(b, s, d, t), None, None, (2,), 0, 3, None, True, True, 1e-3)
            z_hat = z_hat.reshape(b, s * d, t)
        assert z_hat.shape[1] == s * d, (z_hat.shape[1], s * d)
        if self.negatives_mode == 'batch':
            log_batch_mask = self._log_batch_mask(batch_labels, b, z.device)
            targets = torch.arange(b)[:, None]
        elif self.negatives_mode == 'time':
            log_batch_mask = None
            targets = torch.arange(t)[None]
        elif self.negatives_mode == 'all':
            log_batch_mask = None
            targets = torch.arange(b)[:, None] * t + torch.arange(t)
        else:
            raise ValueError(f'Unknown negatives_mode {self.negatives_mode}')
        stats = contrastive_scores(z_hat, z, self.prediction_steps, self.negatives_mode, self.temperature, self.negative_to_target_dist,
                                   log_batch_mask, self.negative_ratio, dense=self.dense_logits)
        return stats, targets.to(z.device)

    def forward(self, inputs):
        x = inputs[self.input_key]
        seq_len = inputs[self.input_seq_len_key]
        x, z, seq_len_z = self.encode(x, seq_len_x=seq_len, target_shape=inputs.get(f'{self.prefix}target_shape', None))
        if self.multi_view:
            z_, z = torch.split(z, z.shape[0] // 2)
            seq_len_z = seq_len_z[:z_.shape[0]]
            z_hat = self.predict(z_, seq_len_z)
        else:
            z_hat = self.predict(z, seq_len_z)
        batch_labels = inputs[self.batch_mask_key] if self.batch_mask_key is not None else None
        stats, targets = self.contrast(z_hat, z, batch_labels)
        return stats, targets, seq_len_z, x

    def review(self, inputs, outputs):
        stats, targets, seq_len_z, x = outputs
        time_labels = inputs[self.time_mask_key] if self.time_mask_key is not None else None
        if self.multi_view:
            x, x_targets = torch.split(x, x.shape[0] // 2)
        else:
            x_targets = x
        accuracies = {}
        negatives = {}
        ce = 0.
        for step, stats_s in zip(self.prediction_steps, stats):
            seq_len_s = np.array(seq_len_z) - abs(step)
            ce_s, hits = stats_s.ce, stats_s.hits
            if time_labels is not None:
                time_mask = (time_labels[:, :-abs(step)] & time_labels[:, abs(step):]).float().to(ce_s.device)
                ce_s = ce_s * time_mask
                hits = hits * time_mask
                accuracy_correction = torch.from_numpy(seq_len_s / (time_mask.sum(1).cpu().numpy() + 1)).to(ce_s.device)
                active_batch_size = np.maximum(torch.sum(time_mask.sum(1) > 0).cpu().numpy(), 1)
            else:
                accuracy_correction = 1.
                active_batch_size = ce_s.shape[0]
            ce = ce + Mean(axis=1)(ce_s, seq_len_s).mean()
            accuracies[f'step_{step}_accuracy'] = (Mean(axis=1)(hits, seq_len_s) * accuracy_correction).cpu().numpy().sum() / active_batch_size
            negatives[f'step_{step}_negatives'] = (stats_s.finite.cpu().numpy() - 1).mean()
        ce = ce / len(self.prediction_steps)
        review = dict(
            losses=dict(ce=ce),
            scalars=dict(overall_accuracy=np.mean(list(accuracies.values())), **accuracies, **negatives),
            histograms=dict(),
            images=dict(input_features=x[:3], target_features=x_targets[:3]),
        )
        return {key1: {f'{self.prefix}{key2}': value for key2, value in d.items()} for key1, d in review.items()}

    def modify_summary(self, summary):
        for key in [f'{self.prefix}input_features', f'{self.prefix}target_features']:
            if key not in summary['images']:
                continue
            from torchvision.utils import make_grid      # (lazily: torchvision is optional)
            image = summary['images'][key]
            if image.dim() == 3:
                image = image.unsqueeze(1)
            summary['images'][key] = make_grid(image.flip(2), normalize=True, scale_each=False, nrow=1)
        return summary

    def get_posteriors(self, outputs):
        stats, targets, seq_len_z, *_ = outputs
        posteriors = []
        with torch.no_grad():
            for step, stats_s in zip(self.prediction_steps, stats):
                seq_len_s = np.array(seq_len_z) - abs(step)
                posteriors.append(Mean(axis=1)(torch.exp(-stats_s.ce.detach()), seq_len_s))     # softmax at the target = exp(-ce)
        posteriors = torch.stack(posteriors, dim=1)
        posteriors = posteriors * np.sqrt(posteriors.shape[0])
        return posteriors.mean(1)


class CPCFeatureExtractor(pt_base.Module):
    def __init__(self, cpc):
        super().__init__()
        self.cpc = cpc

    def forward(self, x, seq_len=None):
        with torch.no_grad():
            x, seq_len = self.cpc.feature_extractor(x, seq_len)
            if isinstance(self.cpc.encoder, (CNN1d, CNNTranspose1d)) and x.dim() != 3:
                assert x.dim() == 4, x.dim()
                x = CPC1d._merge_features(x)
            z, seq_len_z = self.cpc.encoder(x, seq_len)
            if z.dim() == 4:
                z = CPC1d._merge_features(z)
            return z, seq_len_z
