from .modul import MaskEstimator, MaskKeys  # noqa: F401
from .model import MaskEstimatorModel, MaskLossKeys  # noqa: F401
