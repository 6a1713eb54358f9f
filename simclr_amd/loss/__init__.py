from .barlow import BarlowTwins, barlow_twins_torch  # noqa: F401
from .nnclr import NNCLR, nnclr_torch  # noqa: F401
