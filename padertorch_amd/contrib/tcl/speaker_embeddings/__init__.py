from .dvectors import DVectorModel, ResNet18, ResNet34  # noqa: F401
from .loss import AngularPenaltySMLoss  # noqa: F401
