"""``Vocoder``: waveform synthesis from a log-mel spectrogram with a BigVGAN generator (reference:
``padertorch/contrib/mk/synthesis/vocoder/bigvgan.py``).

The reference's constructor and vocoder-tag arithmetic (``bigvgan[_<version>]_<sampling_rate>khz_<mel_bands>band[_<fmax>k]
[_<upsampling_ratio>x]``); the model is read from ``base_dir / vocoder_tag`` (``config.json`` and ``bigvgan_generator.pt``) and never
downloaded: a missing directory raises ``FileNotFoundError``.  The generator runs on the HIP kernels only, so ``device`` has to be the GPU
by the time :meth:`Vocoder.__call__` runs."""
import os
import tempfile
import typing as tp
from pathlib import Path

import numpy as np
import torch

from ..base import Synthesis
from .nvidia_bigvgan import bigvgan

__all__ = ['Vocoder']


class Vocoder(Synthesis):
    """
    Attributes:
        sampling_rate (int): Sampling rate of the training data the vocoder was trained on.
    """

    def __init__(
        self,
        base_dir: tp.Optional[tp.Union[str, Path]] = os.environ.get('BIGVGAN_BASE_DIR', None),
        vocoder_tag: tp.Optional[str] = None,
        version: tp.Optional[str] = 'v2',
        sampling_rate: tp.Optional[int] = 44_000,
        mel_bands: tp.Optional[int] = 128,
        fmax: tp.Optional[int] = None,
        upsampling_ratio: tp.Optional[int] = 256,
        device: tp.Union[str, int] = 'cpu',
        batch_axis: int = 0,
        sequence_axis: int = -1,
        postprocessing: tp.Optional[tp.Callable] = None,
        use_cuda_kernel: bool = False,
    ):
        """
        Args:
            base_dir: Folder that holds one directory per vocoder tag (default: ``$BIGVGAN_BASE_DIR``, else ``<tmp>/bigvgan_models``)
            vocoder_tag: The directory's name; built from the following arguments when None
            version, sampling_rate, mel_bands, fmax, upsampling_ratio: the parts of the tag
            device: Device the generator is moved to
            batch_axis: Axis along which the batches are stacked (ignored for 2-dimensional input)
            sequence_axis: Axis that contains time information
            postprocessing: Optional function applied to every synthesized waveform
            use_cuda_kernel: accepted for compatibility; the activations always run fused
        """
        super().__init__(postprocessing=postprocessing)
        self.base_dir = base_dir
        self.vocoder_tag = vocoder_tag
        self.device = device
        self.batch_axis = batch_axis
        self.sequence_axis = sequence_axis

        if self.vocoder_tag is None:
            self.vocoder_tag = 'bigvgan'
            if version is not None:
                self.vocoder_tag += '_' + version
            self.vocoder_tag += f'_{sampling_rate // 1000}khz_{mel_bands}band'
            if fmax is not None:
                self.vocoder_tag += f'_{fmax // 1000}k'
            if upsampling_ratio is not None:
                self.vocoder_tag += f'_{upsampling_ratio}x'
        if self.base_dir is None:
            self.base_dir = Path(tempfile.gettempdir()) / 'bigvgan_models'
        else:
            self.base_dir = Path(self.base_dir)

        self.vocoder_model = bigvgan.BigVGAN.from_pretrained(self.base_dir / self.vocoder_tag, use_cuda_kernel=use_cuda_kernel)
        self.vocoder_model.remove_weight_norm()
        self.vocoder_model.to(self.device).eval()

        self.vocoder_params = self.vocoder_model.h
        self.sampling_rate = self.vocoder_params.sampling_rate

    def __call__(
        self,
        mel_spec: tp.Union[torch.Tensor, np.ndarray],
        sequence_lengths: tp.Optional[tp.List[int]] = None,
        target_sampling_rate: tp.Optional[int] = None,
    ):
        """Synthesize waveforms from a log-mel spectrogram.

        Args:
            mel_spec: ``[features, time]`` (any order: ``sequence_axis``) or a batch of them (``batch_axis``, ``sequence_axis``)
            sequence_lengths: frames per example of a batch; every example is cut to its length and synthesized on its own
            target_sampling_rate: as :class:`~..base.Synthesis`

        Returns: what went in comes out - a tensor or an array: ``[T]`` for 2-dimensional input, ``[batch, T]`` for a batch, or a list of
            signals where their lengths differ.
        """
        to_numpy = isinstance(mel_spec, np.ndarray)
        if to_numpy:
            mel_spec = torch.from_numpy(mel_spec)
        mel_spec = mel_spec.to(self.device)
        if mel_spec.ndim not in (2, 3):
            raise TypeError(f'Expected 2- or 3-dim. spectrogram but got {mel_spec.ndim}-dim. input with shape {mel_spec.shape}')
        sequence_axis = self.sequence_axis % mel_spec.ndim

        def leave(y):
            return y.detach().cpu().numpy() if to_numpy else y

        with torch.inference_mode():
            if mel_spec.ndim == 2:
                mel_spec = torch.moveaxis(mel_spec, sequence_axis, -1).unsqueeze(0)
                y = leave(self.vocoder_model(mel_spec).view(-1))                     # (T,)
            else:
                batch_axis = self.batch_axis % mel_spec.ndim
                if batch_axis == sequence_axis:
                    raise ValueError(f'batch_axis {self.batch_axis} and sequence_axis {self.sequence_axis} are the same axis')
                feature_axis = ({0, 1, 2} - {batch_axis, sequence_axis}).pop()
                mel_spec = mel_spec.permute(batch_axis, feature_axis, sequence_axis)  # b f t
                if sequence_lengths is None:
                    sequence_lengths = [mel_spec.shape[-1]] * mel_spec.shape[0]
                y = [leave(self.vocoder_model(m.unsqueeze(0)[..., :seq_len]).view(-1)) for m, seq_len in zip(mel_spec, sequence_lengths)]
                try:
                    y = np.stack(y) if to_numpy else torch.stack(y)
                except (ValueError, RuntimeError):
                    pass                                                             # signals of different lengths stay a list
        return super().__call__(y, target_sampling_rate)
