from .wavenet import WaveNet, Conv  # noqa: F401
