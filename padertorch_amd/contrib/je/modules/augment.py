"""Data augmentation on feature tensors (reference: ``padertorch/contrib/je/modules/augment.py``).

Every class keeps the reference's constructor and ``training`` semantics and draws its random quantities ON THE HOST, from the same
streams in the same order as the reference (numpy's global generator, torch's CPU generator, the user's sampling functions), so a seeded
run matches a seeded reference run.  The draws are made by a ``draw`` method per class; ``forward`` hands them to one launch of the
feature kernels (``ops/je_features.py``) with every other stage switched off, and ``NormalizedLogMelExtractor`` calls the ``draw``
methods itself and fuses the stages.  Only ``randn_like`` of ``AdditiveNoise`` runs on the device.

``TimeWarping``, ``GaussianBlur2d``, ``Mixup``, ``Mask`` and ``AdditiveNoise`` take a float32 ``[B, C, F, T]`` tensor on the GPU;
``Scale`` / ``Shift`` are one device multiply / add and ``Superpose`` is the reference's torch ops (inside the extractor it is part of
the log-mel kernel).
"""
import numpy as np
import torch
from torch import nn

from ....ops import je_features as _ops

__all__ = ['Scale', 'Shift', 'TimeWarping', 'Superpose', 'Mixup', 'Mask', 'AdditiveNoise', 'GaussianBlur2d', 'TruncatedExponential',
           'get_gaussian_kernel1d', 'get_gaussian_kernel2d', 'gaussian']


def _per_example(values, x):
    values = torch.as_tensor(np.asarray(values)).float()
    return values[(...,) + (x.dim() - 1) * (None,)].to(x.device)


class TruncatedExponential:
    """``loc + Exp(scale)`` truncated to ``[loc, loc + truncation]`` - the sampler the extractor builds for the blur's sigma (paderbox's
    ``random_utils.TruncatedExponential`` in the reference; restated, parity unpinned).  Draws from numpy's global generator."""

    def __init__(self, loc=0., scale=1., truncation=3.):
        self.loc, self.scale, self.truncation = loc, scale, truncation

    def __call__(self, size=None):
        from scipy.stats import truncexpon
        return truncexpon(self.truncation / self.scale, loc=self.loc, scale=self.scale).rvs(size)


class Scale(nn.Module):
    def __init__(self, scale_sampling_fn):
        super().__init__()
        self.scale_sampling_fn = scale_sampling_fn

    def draw(self, B):
        return np.asarray(self.scale_sampling_fn(B))

    def forward(self, x):
        if not self.training:
            return x
        return x * _per_example(self.draw(x.shape[0]), x)


class Shift(nn.Module):
    def __init__(self, shift_sampling_fn):
        super().__init__()
        self.shift_sampling_fn = shift_sampling_fn

    def draw(self, B):
        return np.asarray(self.shift_sampling_fn(B))

    def forward(self, x):
        if not self.training:
            return x
        return x + _per_example(self.draw(x.shape[0]), x)


class TimeWarping(nn.Module):
    """``warping_fn(seq_len) -> (time_indices [B, T'], seq_len)``; frame ``t`` of the output interpolates linearly between the frames
    ``floor`` and ``ceil`` of ``time_indices[b, t]`` (``augment.py:84-122``)."""

    def __init__(self, warping_fn, batch_axis=0, sequence_axis=-1):
        super().__init__()
        self.warping_fn = warping_fn
        self.batch_axis = batch_axis
        self.sequence_axis = sequence_axis

    def draw(self, seq_len):
        assert seq_len is not None
        time_indices, seq_len = self.warping_fn(seq_len)
        return np.asarray(time_indices, dtype=np.float64), seq_len

    def forward(self, *tensors, seq_len):
        if not self.training:
            return (*tensors, seq_len)
        time_indices, seq_len = self.draw(seq_len)
        for t in tensors:
            if t.dim() != 4 or self.batch_axis != 0 or self.sequence_axis % t.dim() != 3:
                raise NotImplementedError('TimeWarping covers [B, C, F, T] tensors with the batch axis first and the sequence axis last')
        return (*[_ops.feature_shape(t, time_indices=time_indices) for t in tensors], seq_len)


def _mix_targets(targets, lambda_, shuffle_idx, fn):
    if targets is None:
        return None
    if isinstance(targets, (list, tuple)):
        return [_mix_targets(t, lambda_, shuffle_idx, fn) for t in targets]
    lam = torch.from_numpy(np.asarray(lambda_)).float().to(targets.device)
    return fn(targets, lam[(...,) + (targets.dim() - 1) * (None,)], targets[torch.as_tensor(shuffle_idx, device=targets.device)])


class Superpose(nn.Module):
    def __init__(self, p, scale_fn=None):
        super().__init__()
        self.p = p
        self.scale_fn = scale_fn

    def draw(self, B, seq_len=None):
        """``(shuffle_idx, lambda, gain, partner_gain, seq_len)`` in the reference's order: roll, lambda, then one scale draw for ``x``
        and one for the shuffled ``x`` (``None`` without a scale function)."""
        if B < 2:
            raise NotImplementedError(f'Superpose needs B >= 2 examples (got B = {B}), as in the reference')
        shuffle_idx = np.roll(np.arange(B, dtype=np.int64), np.random.choice(B - 1) + 1)
        lambda_ = np.random.binomial(1, self.p, B)
        if seq_len is not None:
            seq_len = np.maximum(seq_len, (lambda_ > 0.) * np.array(seq_len)[shuffle_idx])
        gain = partner_gain = None
        if self.scale_fn is not None and self.scale_fn.training:
            gain = self.scale_fn.draw(B)
            partner_gain = self.scale_fn.draw(B)
        return shuffle_idx, lambda_, gain, partner_gain, seq_len

    @staticmethod
    def mix_targets(targets, lambda_, shuffle_idx):
        return _mix_targets(targets, lambda_, shuffle_idx, lambda t, lam, ts: t + lam * (1 - t) * ts)

    def forward(self, x, targets, seq_len=None):
        if self.training:
            shuffle_idx, lambda_, gain, partner_gain, seq_len = self.draw(x.shape[0], seq_len)
            x_shuffled = x[torch.as_tensor(shuffle_idx, device=x.device)]
            if gain is not None:
                x, x_shuffled = x * _per_example(gain, x), x_shuffled * _per_example(partner_gain, x)
            x = x + _per_example(lambda_, x) * x_shuffled
            targets = self.mix_targets(targets, lambda_, shuffle_idx)
        return x, targets, seq_len


class Mixup(nn.Module):
    def __init__(self, p, alpha=1.):
        super().__init__()
        self.p = p
        self.alpha = alpha

    def draw(self, B, seq_len=None):
        shuffle_idx = np.roll(np.arange(B, dtype=np.int64), np.random.choice(B))
        lambda_ = np.maximum(np.random.binomial(1, 1 - self.p, B), np.random.beta(self.alpha, self.alpha, B))
        if seq_len is not None:
            seq_len = np.maximum(seq_len, (lambda_ < 1.) * np.array(seq_len)[shuffle_idx])
        assert all(lambda_ >= 0.) and all(lambda_ <= 1.)
        return shuffle_idx, lambda_, seq_len

    @staticmethod
    def mix_targets(targets, lambda_, shuffle_idx):
        return _mix_targets(targets, lambda_, shuffle_idx, lambda t, lam, ts: lam * t + (1. - lam) * ts)

    def forward(self, x, targets=None, seq_len=None):
        if self.training:
            shuffle_idx, lambda_, seq_len = self.draw(x.shape[0], seq_len)
            x = _ops.feature_tail(x, partner=shuffle_idx, lam=lambda_)
            targets = self.mix_targets(targets, lambda_, shuffle_idx)
        return x, targets, seq_len


class Mask(nn.Module):
    def __init__(self, axis, n_masks=1, max_masked_steps=None, max_masked_rate=1.):
        super().__init__()
        self.axis = axis
        self.n_masks = n_masks
        self.max_masked_values = max_masked_steps
        self.max_masked_rate = max_masked_rate

    def draw(self, B, size, seq_len=None):
        """``(onset, offset)`` int32 ``[n_masks, B]`` from two ``torch.rand(B)`` per mask and the reference's float32 floor arithmetic
        (``augment.py:222-236``); ``size``: the masked axis' length, which stands in for a missing ``seq_len``."""
        seq_len = size * torch.ones(B) if seq_len is None else torch.Tensor(np.asarray(seq_len, dtype=np.float64))
        max_width = self.max_masked_rate / self.n_masks * seq_len
        if self.max_masked_values is not None:
            max_width = torch.min(self.max_masked_values * torch.ones_like(max_width) / self.n_masks, max_width)
        max_width = torch.floor(max_width)
        onsets, offsets = [], []
        for _ in range(self.n_masks):
            width = torch.floor(torch.rand(B) * (max_width + 1))
            onset = torch.floor(torch.rand(B) * (seq_len - width + 1))
            onsets.append(onset)
            offsets.append(onset + width)
        # index < onset and index >= offset on float values of whole numbers: the same as on integers
        return torch.stack(onsets).numpy().astype(np.int32), torch.stack(offsets).numpy().astype(np.int32)

    def forward(self, x, seq_len=None):
        if not self.training:
            return x
        axis = self.axis % x.dim()
        if x.dim() != 4 or axis < 2:
            raise NotImplementedError('Mask covers the frequency (-2) and time (-1) axes of a [B, C, F, T] tensor')
        tables = self.draw(x.shape[0], x.shape[axis], seq_len)
        return _ops.feature_tail(x, **{'time_masks' if axis == 3 else 'freq_masks': tables})


class AdditiveNoise(nn.Module):
    def __init__(self, max_scale):
        super().__init__()
        self.max_scale = max_scale

    def draw(self, B):
        return torch.rand(B) * self.max_scale

    def forward(self, x):
        if not self.training:
            return x
        return _ops.feature_tail(x, noise_scale=self.draw(x.shape[0]), noise=torch.randn_like(x))


class GaussianBlur2d(nn.Module):
    """Blurs every example of a ``[B, C, H, W]`` tensor with its own ``kernel_size x kernel_size`` Gaussian (sigma from
    ``sigma_sampling_fn(B)``) over the reflect-padded plane (``augment.py:258-336``).  ``'reflect'`` is the padding the kernel has."""

    def __init__(self, kernel_size, sigma_sampling_fn, pad_mode: str = 'reflect'):
        super().__init__()
        self.kernel_size = kernel_size
        self.sigma_sampling_fn = sigma_sampling_fn
        if pad_mode != 'reflect':
            raise NotImplementedError(f'GaussianBlur2d covers pad_mode "reflect" only, got "{pad_mode}"')
        self.pad_mode = pad_mode

    def __repr__(self) -> str:
        return (f'{self.__class__.__name__}(kernel_size={self.kernel_size}, sigma_sampling_fn={self.sigma_sampling_fn!r}, '
                f'border_type={self.pad_mode})')

    def draw(self, B):
        """The 1-D taps ``[B, kernel_size]`` (float32, host); the 2-D kernel is their outer product."""
        sigma = torch.from_numpy(np.array(self.sigma_sampling_fn(B))).float()
        return get_gaussian_kernel1d(self.kernel_size, sigma)

    def forward(self, x):
        if not x.dim() == 4:
            raise ValueError(f'Invalid input shape, we expect BxCxHxW. Got: {x.shape}')
        if not self.training:
            return x
        return _ops.feature_shape(x, taps=self.draw(x.shape[0]))


def get_gaussian_kernel2d(kernel_size, sigma, force_even: bool = False):
    kernel_1d = get_gaussian_kernel1d(kernel_size, sigma, force_even)
    return kernel_1d.unsqueeze(-1) @ kernel_1d.unsqueeze(-2)


def get_gaussian_kernel1d(kernel_size: int, sigma, force_even: bool = False) -> torch.Tensor:
    if not isinstance(kernel_size, int) or (kernel_size % 2 == 0 and not force_even) or kernel_size <= 0:
        raise TypeError(f'kernel_size must be an odd positive integer. Got {kernel_size}')
    return gaussian(kernel_size, sigma)


def gaussian(window_size, sigma):
    x = torch.arange(window_size).float() - window_size // 2
    if torch.is_tensor(sigma) and sigma.dim() > 0:
        sigma = sigma[..., None]
    if window_size % 2 == 0:
        x = x + 0.5
    gauss = torch.exp((-x.pow(2.0) / (2 * sigma ** 2))).float()
    return gauss / gauss.sum(-1, keepdim=True)
