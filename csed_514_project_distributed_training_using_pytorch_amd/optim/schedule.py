"""Device-resident learning-rate schedules.

A schedule is an fp32 **table** ``lr[t]``, one entry per optimizer step, and an int64 **position**
``t``; steps past the end of the table train at its last entry.  Both live on the device: the kernel
that applies SGD (``csed::lenet_update`` / ``csed::sgd_flat``) reads ``table[min(t, len - 1)]`` for
its own step and its last block advances ``t``, so the steps of one captured HIP graph (or of one
native-executor run) train at different rates with no host in between, and one capture serves the
whole schedule.

A table rather than closed-form device math: any schedule can be expressed (``from_torch`` tabulates
every ``torch.optim.lr_scheduler``), and the device uses bit for bit the fp32 value the host computed
-- the scheduled step is bitwise the constant-lr step at that value.
"""
from __future__ import annotations

import warnings
from typing import Callable

import torch

from ..ops import _native


class LRSchedule:
    def __init__(self, table, t: int = 0):
        table = torch.as_tensor(table, dtype=torch.float32).detach().reshape(-1).clone()
        if table.numel() < 1:
            raise ValueError("LRSchedule needs at least one table entry")
        self.table = table.contiguous()
        self.pos = torch.full((1,), int(t), dtype=torch.long)

    # ------------------------------------------------------------ constructors
    @classmethod
    def constant(cls, lr: float, steps: int = 1) -> "LRSchedule":
        return cls(torch.full((max(1, int(steps)),), float(lr), dtype=torch.float64))

    @classmethod
    def from_torch(cls, make_scheduler: Callable, base_lr: float, steps: int) -> "LRSchedule":
        """Tabulate ``make_scheduler(optimizer)`` (any ``torch.optim.lr_scheduler``) on a throw-away
        ``torch.optim.SGD(lr=base_lr)``: the ``param_groups[0]["lr"]`` of ``steps`` optimizer steps,
        each rounded once to fp32."""
        if steps < 1:
            raise ValueError("LRSchedule.from_torch: steps >= 1")
        opt = torch.optim.SGD([torch.zeros(1, requires_grad=True)], lr=float(base_lr))
        lrs = []
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")  # (SequentialLR's hand-over uses the deprecated epoch form)
            sched = make_scheduler(opt)
            for _ in range(int(steps)):
                lrs.append(float(opt.param_groups[0]["lr"]))
                opt.step()
                sched.step()
        return cls(torch.tensor(lrs, dtype=torch.float64))

    @classmethod
    def warmup_cosine(cls, base_lr: float, warmup_steps: int, total_steps: int, min_lr: float = 0.0,
                      start_factor: float = 1.0 / 3) -> "LRSchedule":
        """Linear warm-up from ``start_factor * base_lr`` to ``base_lr`` over ``warmup_steps`` steps, then
        half a cosine down to ``min_lr`` at ``total_steps``: step t >= warmup trains at
        ``min_lr + (base_lr - min_lr) * (1 + cos(pi * (t - warmup) / (total - warmup))) / 2``.  By
        definition torch's ``SequentialLR([LinearLR, CosineAnnealingLR], [warmup_steps])`` (tabulated by
        it, so the tables agree element for element)."""
        from torch.optim import lr_scheduler as ls

        warmup_steps, total_steps = int(warmup_steps), int(total_steps)
        if not 0 <= warmup_steps < total_steps:
            raise ValueError("warmup_cosine: 0 <= warmup_steps < total_steps")

        def make(opt):
            cos = lambda: ls.CosineAnnealingLR(opt, T_max=total_steps - warmup_steps, eta_min=float(min_lr))  # noqa: E731
            if warmup_steps == 0:
                return cos()
            lin = ls.LinearLR(opt, start_factor=float(start_factor), end_factor=1.0, total_iters=warmup_steps)
            return ls.SequentialLR(opt, [lin, cos()], milestones=[warmup_steps])

        return cls.from_torch(make, base_lr, total_steps)

    @classmethod
    def warmup_step(cls, base_lr: float, warmup_steps: int, step_size: int, gamma: float, total_steps: int,
                    start_factor: float = 1.0 / 3) -> "LRSchedule":
        """Linear warm-up as in ``warmup_cosine``, then ``base_lr * gamma ** ((t - warmup) // step_size)``:
        torch's ``SequentialLR([LinearLR, StepLR], [warmup_steps])``, tabulated by it."""
        from torch.optim import lr_scheduler as ls

        warmup_steps, total_steps = int(warmup_steps), int(total_steps)
        if not 0 <= warmup_steps < total_steps or step_size < 1:
            raise ValueError("warmup_step: 0 <= warmup_steps < total_steps, step_size >= 1")

        def make(opt):
            stp = lambda: ls.StepLR(opt, step_size=int(step_size), gamma=float(gamma))  # noqa: E731
            if warmup_steps == 0:
                return stp()
            lin = ls.LinearLR(opt, start_factor=float(start_factor), end_factor=1.0, total_iters=warmup_steps)
            return ls.SequentialLR(opt, [lin, stp()], milestones=[warmup_steps])

        return cls.from_torch(make, base_lr, total_steps)

    # ----------------------------------------------------------------- device
    def __len__(self) -> int:
        return self.table.numel()

    @property
    def device(self) -> torch.device:
        return self.table.device

    def to(self, device) -> "LRSchedule":
        """Table and position on ``device`` (in place; returns self).  Buffers come from the extension's
        own zero fill plus copies: no torch fill kernel in an engine's bring-up."""
        device = torch.device(device)
        if device.type == "cuda" and device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        if self.table.device != device:
            table = _native.zeros(self.table.shape, torch.float32, device)
            pos = _native.zeros(1, torch.long, device)
            table.copy_(self.table)
            pos.copy_(self.pos)
            self.table, self.pos = table, pos
        return self

    def position(self) -> int:
        """The number of optimizer steps taken on this schedule (one host sync)."""
        return int(self.pos.item())

    def set_position(self, t: int) -> None:
        self.pos.copy_(torch.full((1,), int(t), dtype=torch.long))

    def current_lr(self) -> float:
        """The rate of the next optimizer step: ``table[min(t, len - 1)]`` (one host sync)."""
        t = min(max(self.position(), 0), len(self) - 1)
        return float(self.table[t].item())

    # ------------------------------------------------------------------ state
    def state_dict(self) -> dict:
        return {"table": self.table.detach().cpu().clone(), "t": self.position()}

    def load_state_dict(self, sd: dict) -> None:
        """Table and position of ``sd``, kept on this schedule's device.  A table of the same length is
        copied into the existing buffer (captured graphs that point at it stay valid)."""
        table = torch.as_tensor(sd["table"], dtype=torch.float32).reshape(-1)
        if table.numel() < 1:
            raise ValueError("LRSchedule needs at least one table entry")
        if table.numel() == self.table.numel():
            self.table.copy_(table)
        else:
            dev = self.table.device
            self.table = table.clone().contiguous()
            self.pos = self.pos.cpu()
            self.to(dev)
        self.set_position(int(sd["t"]))

    @classmethod
    def from_state_dict(cls, sd: dict) -> "LRSchedule":
        return cls(sd["table"], int(sd["t"]))
