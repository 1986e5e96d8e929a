"""Optimizers: SGD-momentum as one fused HIP kernel over a flat buffer, Adam / AdamW over a flat buffer on CPU
parameters, device-resident LR schedules."""
from .adam import FusedAdam
from .schedule import LRSchedule
from .sgd import FusedSGD

__all__ = ["FusedAdam", "FusedSGD", "LRSchedule"]
