"""Optimizers: SGD-momentum as one fused HIP kernel over a flat buffer, Adam / AdamW over a flat buffer on CPU
parameters, device-resident LR schedules, global-norm gradient clipping as a HIP kernel on the flat gradient."""
from .adam import FusedAdam
from .clip import ClipPlan, GradClip, clip_plan
from .schedule import LRSchedule
from .sgd import FusedSGD

__all__ = ["ClipPlan", "FusedAdam", "FusedSGD", "GradClip", "LRSchedule", "clip_plan"]
