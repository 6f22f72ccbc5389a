"""``padertorch.contrib.mk`` on the HIP path: ``synthesis`` (spectrogram -> waveform)."""
from . import synthesis  # noqa: F401
