"""``padertorch.contrib.mk.synthesis.vocoder``: of the neural vocoders, BigVGAN - the generator and its anti-aliased activation
(:mod:`.nvidia_bigvgan`) and the :class:`Vocoder` that wraps a local checkpoint of it (:mod:`.bigvgan`)."""
from . import nvidia_bigvgan  # noqa: F401
from .bigvgan import Vocoder  # noqa: F401
