"""Optimizers: SGD-momentum as one fused HIP kernel over a flat buffer, device-resident LR schedules."""
from .schedule import LRSchedule
from .sgd import FusedSGD

__all__ = ["FusedSGD", "LRSchedule"]
