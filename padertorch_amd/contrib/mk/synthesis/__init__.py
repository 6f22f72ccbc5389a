"""``padertorch.contrib.mk.synthesis``: the parametric synthesis (fast Griffin-Lim).  The neural vocoders of the reference package are
not part of this project, except BigVGAN's anti-aliased activation (:mod:`.vocoder.nvidia_bigvgan`)."""
from . import vocoder  # noqa: F401
from .base import Synthesis
from .parametric import FGLA, fast_griffin_lim, griffin_lim_step

__all__ = ['Synthesis', 'FGLA', 'fast_griffin_lim', 'griffin_lim_step']
