from .model import OneAndRestPIT  # noqa: F401
from .....ops.orpit import one_and_rest_permutation_invariant_loss  # noqa: F401
