from . import regression
from . import source_separation
from .regression import *  # noqa: F401,F403
from .source_separation import *  # noqa: F401,F403
from .source_separation import pit_mse_ips_losses, dc_loss_batched  # noqa: F401
from ..orpit import one_and_rest_permutation_invariant_loss  # noqa: F401,E402
from ..mask_loss import mask_bce_loss  # noqa: F401,E402
