from .griffin_lim import FGLA, fast_griffin_lim, griffin_lim_step

__all__ = ['FGLA', 'fast_griffin_lim', 'griffin_lim_step']
