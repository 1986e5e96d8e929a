"""Adam / AdamW over a flat parameter buffer, for CPU parameters: the rule the fused engine's update kernel
applies (``lenet_update``'s ``adam_step`` / ``adam_rule``), evaluated operation for operation in float32 torch.

Drop-in for ``torch.optim.Adam(params, lr, betas, eps, weight_decay)`` and, with ``decoupled=True``, for
``torch.optim.AdamW`` (``amsgrad=False``, ``maximize=False``, one parameter group): the same rule, torch's own
``param_groups`` and the same ``state_dict()`` layout (``state[i]['step' | 'exp_avg' | 'exp_avg_sq']``), so
``results/optimizer.pth`` files are interchangeable with stock PyTorch.

The counterpart of :class:`FusedSGD`'s CPU path (oracle and plumbing): both moments are flat buffers beside the
parameters, the exact step number is a tensor, an :class:`LRSchedule` supplies the rate of each step.  There is
no flat Adam kernel for the per-op engine yet, so GPU parameters are refused instead of being stepped with torch
kernels; on a GPU Adam runs in the fused engine.
"""
from __future__ import annotations

import math

import torch

from ..utils.flat import FlatParams
from .schedule import LRSchedule


class FusedAdam(torch.optim.Adam):
    def __init__(self, params, lr: float = 1e-3, betas: tuple[float, float] = (0.9, 0.999), eps: float = 1e-8,
                 weight_decay: float = 0.0, decoupled: bool = False, flat: FlatParams | None = None):
        params = list(params)
        if any(isinstance(p, torch.Tensor) and p.device.type != "cpu" for p in params):  # (before anything is re-homed)
            raise NotImplementedError("FusedAdam steps CPU parameters only: the per-op engine has no flat Adam "
                                      "kernel (use the fused engine's optimizer=\"adam\" | \"adamw\" on a GPU)")
        super().__init__(params, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay,
                         decoupled_weight_decay=bool(decoupled))
        if len(self.param_groups) != 1:
            raise ValueError("FusedAdam supports a single parameter group")
        plist = self.param_groups[0]["params"]
        self.flat = flat if flat is not None else FlatParams(plist)
        if [id(p) for p in self.flat.params] != [id(p) for p in plist]:
            raise ValueError("flat buffer parameters must match the optimizer parameters (same order)")
        dev = self.flat.device
        self.exp_avg_flat = torch.zeros_like(self.flat.data)
        self.exp_avg_sq_flat = torch.zeros_like(self.flat.data)
        self.step_count = torch.zeros(1, dtype=torch.long, device=dev)  # steps taken: the next one is t = count + 1
        self.grad_scale = 1.0
        self.lr_schedule: LRSchedule | None = None

    @property
    def decoupled(self) -> bool:
        return bool(self.param_groups[0].get("decoupled_weight_decay", False))

    @property
    def name(self) -> str:
        return "adamw" if self.decoupled else "adam"

    def set_lr_schedule(self, schedule: LRSchedule | None) -> None:
        """Train at ``schedule``'s rates from its current position instead of ``param_groups[0]["lr"]``; None
        returns to the param group's value."""
        self.lr_schedule = None if schedule is None else schedule.to(self.flat.device)

    def zero_grad(self, set_to_none: bool = True) -> None:  # noqa: D401 - torch signature
        """Zero the flat gradient in one fill; grads stay views of the flat buffer."""
        self.flat.zero_grad()

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        g = self.param_groups[0]
        self.flat.gather_grads()
        self._cpu_step(g)
        return loss

    def _cpu_step(self, g) -> None:
        """The fused engine's rule in plain float32 torch operations (bias corrections from float32 log(beta) formed
        in double, the product and expm1 in float32)."""
        f = lambda x: torch.tensor(float(x), dtype=torch.float32)  # noqa: E731
        lr = g["lr"]
        if self.lr_schedule is not None:
            lr = self.lr_schedule.current_lr()
            self.lr_schedule.pos += 1
        lr, b1, b2, eps, wd = f(lr), f(g["betas"][0]), f(g["betas"][1]), f(g["eps"]), f(g["weight_decay"])
        t, one = f(int(self.step_count.item()) + 1), f(1.0)
        lb = [f(math.log(float(b))) if float(b) > 0.0 else f(-math.inf) for b in (b1, b2)]
        step_size = lr / -torch.expm1(t * lb[0])
        bc2_sqrt = (-torch.expm1(t * lb[1])).sqrt()
        p, m, v = self.flat.data, self.exp_avg_flat, self.exp_avg_sq_flat
        d = self.flat.grad * f(self.grad_scale)
        if self.decoupled:
            p.mul_(one - lr * wd)
        else:
            d = d + wd * p
        m.add_((one - b1) * (d - m))
        v.mul_(b2).add_((one - b2) * (d * d))
        p.sub_(step_size * (m / (v.sqrt() / bc2_sqrt + eps)))
        self.step_count += 1

    # ---- torch.optim.Adam-compatible state dict ------------------------------------------------
    def state_dict(self):
        """What torch.optim.Adam / AdamW (amsgrad=False) of this torch return: per parameter the step number (a
        float32 scalar, theirs) and both moments, empty before the first step; under a schedule the group's
        ``lr`` is the current rate (what a torch scheduler leaves there)."""
        sd = super().state_dict()  # (self.state stays empty: the flat buffers are the state; torch's groups)
        t = int(self.step_count.item())
        if t > 0:
            for i in range(len(self.flat.params)):
                sd["state"][i] = {"step": torch.tensor(float(t), dtype=torch.float32),
                                  "exp_avg": self.flat.view(self.exp_avg_flat, i).detach().clone(),
                                  "exp_avg_sq": self.flat.view(self.exp_avg_sq_flat, i).detach().clone()}
        if self.lr_schedule is not None:
            sd["param_groups"][0]["lr"] = self.lr_schedule.current_lr()
        return sd

    def load_state_dict(self, state_dict):
        g = state_dict["param_groups"][0]
        if "betas" not in g:
            raise ValueError(f"this optimizer state is not Adam's (its group has {sorted(g)}): the optimizer "
                             f"trains with {self.name}")
        if bool(g.get("decoupled_weight_decay", False)) != self.decoupled:
            raise ValueError(f"this optimizer state is {'AdamW' if g.get('decoupled_weight_decay') else 'Adam'}'s, "
                             f"the optimizer trains with {self.name}")
        if g.get("amsgrad"):
            raise ValueError("amsgrad optimizer states are not supported")
        super().load_state_dict(state_dict)
        t = 0
        with torch.no_grad():
            self.exp_avg_flat.zero_()
            self.exp_avg_sq_flat.zero_()
            for i, p in enumerate(self.flat.params):
                st = self.state.get(p)
                if st:
                    self.flat.view(self.exp_avg_flat, i).copy_(st["exp_avg"])
                    self.flat.view(self.exp_avg_sq_flat, i).copy_(st["exp_avg_sq"])
                    t = int(st["step"])
            self.step_count.fill_(t)  # (the exact step: the bias corrections continue where the file left off)
        self.state.clear()  # (torch's per-parameter copies: the flat buffers hold the state from here on)
