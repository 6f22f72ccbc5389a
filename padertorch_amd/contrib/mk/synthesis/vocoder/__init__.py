"""``padertorch.contrib.mk.synthesis.vocoder``: of the neural vocoders, the anti-aliased activation of BigVGAN (:mod:`.nvidia_bigvgan`).
The generators themselves are not part of this project."""
from . import nvidia_bigvgan  # noqa: F401
