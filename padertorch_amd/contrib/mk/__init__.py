"""``padertorch.contrib.mk`` on the HIP path: ``synthesis`` (spectrogram -> waveform) and ``modules`` (contrastive predictive coding)."""
from . import synthesis  # noqa: F401
from . import modules  # noqa: F401
