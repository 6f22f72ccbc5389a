"""``Synthesis``: what every waveform synthesis shares (reference: ``padertorch/contrib/mk/synthesis/base.py``).

A plain class here: ``pt.Configurable`` is out of scope for this project.  Resampling is limited to the identity: the reference
resamples on the host with sox (``paderbox.transform.module_resample.resample_sox``), which this project does not have, so a
``target_sampling_rate`` that differs from ``sampling_rate`` raises ``NotImplementedError``.
"""
import typing
from functools import partial

import numpy as np
import torch

__all__ = ['Synthesis']


class Synthesis:
    sampling_rate: int

    def __init__(self, postprocessing: typing.Optional[typing.Callable] = None):
        self.postprocessing = postprocessing

    def __call__(self, time_signal, target_sampling_rate: typing.Optional[int] = None):
        """``time_signal``: one signal, a ``[batch, T]`` array / tensor or a list of signals; ``postprocessing`` is applied per signal."""
        if self.postprocessing is not None:
            if isinstance(time_signal, list) or time_signal.ndim == 2:
                time_signal = [self.postprocessing(s) for s in time_signal]
            else:
                time_signal = self.postprocessing(time_signal)
        return self.resample(time_signal, target_sampling_rate)

    def _resample(self, wav, target_sampling_rate: typing.Optional[int] = None):
        if target_sampling_rate is None or target_sampling_rate == self.sampling_rate:
            return wav
        raise NotImplementedError(
            f'resampling from {self.sampling_rate} Hz to {target_sampling_rate} Hz: the reference resamples with sox on the host '
            f'(paderbox resample_sox), which padertorch_amd does not have; resample the returned signal yourself')

    def resample(self, wav, target_sampling_rate: typing.Optional[int] = None):
        if isinstance(wav, list) or wav.ndim == 2:
            wav = list(map(partial(self._resample, target_sampling_rate=target_sampling_rate), wav))
            try:
                wav = (np if isinstance(wav[0], np.ndarray) else torch).stack(wav)
            except (ValueError, RuntimeError):
                pass        # signals of different lengths stay a list
            return wav
        return self._resample(wav, target_sampling_rate=target_sampling_rate)
