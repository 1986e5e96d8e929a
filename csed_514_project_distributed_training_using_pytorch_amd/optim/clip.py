"""Global-norm gradient clipping of a flat fp32 gradient on the device (``csed::clip_grad_norm_``,
csrc/kernels/clip.hip): ``torch.nn.utils.clip_grad_norm_`` with the 2-norm, in place, as one launch of one
workgroup up to ``clip_plan(n).one_wg_max`` elements and two launches over a small partial-sum buffer past it.

``GradClip`` is what an optimizer keeps: the clip value, the ``stats`` the kernel leaves on the device
(norm before clipping, coefficient) and the larger form's scratch, sized from the plan the launcher itself
dispatches on.
"""
from __future__ import annotations

from typing import NamedTuple

import torch

from ..ops import _native


class ClipPlan(NamedTuple):
    """``csed::clip_plan``, in its order."""
    form: int        # 0: one workgroup, one launch; 1: partial sums, then the scale
    grid: int        # workgroups of each launch
    partials: int    # floats of scratch the form needs (0: none)
    one_wg_max: int  # largest n of form 0
    threads: int     # threads per workgroup


def clip_plan(n: int) -> ClipPlan:
    return ClipPlan(*(int(v) for v in _native.ops().clip_plan(int(n))))


def check_max_norm(max_norm) -> float | None:
    """``max_norm`` as a float (None: no clipping); it must be a positive number."""
    if max_norm is None:
        return None
    v = float(max_norm)
    if not v > 0.0:
        raise ValueError(f"max_norm {max_norm}: expected a positive value (None switches clipping off)")
    return v


class GradClip:
    """Clips ``grad`` (a contiguous fp32 device tensor or view, kept by address) to ``max_norm``."""

    def __init__(self, grad: torch.Tensor, max_norm: float):
        self.grad, self.max_norm = grad, check_max_norm(max_norm)
        self.stats = _native.zeros(2, torch.float32, grad.device)
        need = clip_plan(grad.numel()).partials
        self.partials = _native.zeros(need, torch.float32, grad.device) if need else None

    def args(self) -> tuple:
        """The arguments of ``csed::clip_grad_norm_``."""
        return (self.grad, self.max_norm, self.stats, self.partials)

    def launch(self) -> None:
        _native.ops().clip_grad_norm_(*self.args())

    def last_norm(self) -> float:
        """The gradient's norm before the last clip (one device read)."""
        return float(self.stats[0].item())
