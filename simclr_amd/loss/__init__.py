from .barlow import BarlowTwins, barlow_twins_torch  # noqa: F401
