from .tas_coders import StftEncoder, IstftDecoder, TasEncoder, TasDecoder  # noqa: F401
from .loss import tasnet_loss  # noqa: F401
from .model import TasNet  # noqa: F401
