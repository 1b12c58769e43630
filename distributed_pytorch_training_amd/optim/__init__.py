from .fused import FusedAdam, FusedLAMB, FusedLARS, FusedSGD, build_optimizer
from .stock import LAMB, LARS

__all__ = ["FusedAdam", "FusedLAMB", "FusedLARS", "FusedSGD", "LAMB", "LARS", "build_optimizer"]
