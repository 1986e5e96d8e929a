"""SGD with momentum as ONE fused HIP kernel over a flat parameter buffer.

Drop-in for ``torch.optim.SGD(params, lr, momentum)`` (ref src/train.py:60-61,
src/train_dist.py:66): same update rule (dampening, weight decay, Nesterov),
same ``param_groups`` and the same ``state_dict()`` layout
(``state[i]['momentum_buffer']``), so ``results/optimizer.pth`` files are
interchangeable with stock PyTorch.

On the GPU the stock non-foreach SGD issues ~3 launches per parameter tensor
(24 for Net); here it is one launch over 21,840 floats.  The "first step"
flag lives on the device (a step counter bumped by the kernel's last block),
so the update is capturable in a HIP graph and replayable.
"""
from __future__ import annotations

import torch

from ..ops import _native
from ..utils.flat import FlatParams
from .schedule import LRSchedule


class FusedSGD(torch.optim.SGD):
    def __init__(self, params, lr: float = 0.01, momentum: float = 0.0, dampening: float = 0.0,
                 weight_decay: float = 0.0, nesterov: bool = False, flat: FlatParams | None = None):
        params = list(params)
        super().__init__(params, lr=lr, momentum=momentum, dampening=dampening, weight_decay=weight_decay,
                         nesterov=nesterov)
        if len(self.param_groups) != 1:
            raise ValueError("FusedSGD supports a single parameter group")
        plist = self.param_groups[0]["params"]
        self.flat = flat if flat is not None else FlatParams(plist)
        if [id(p) for p in self.flat.params] != [id(p) for p in plist]:
            raise ValueError("flat buffer parameters must match the optimizer parameters (same order)")
        dev = self.flat.device
        self.momentum_flat = torch.zeros_like(self.flat.data)
        self.step_count = torch.zeros(1, dtype=torch.long, device=dev)
        self._ticket = torch.zeros(1, dtype=torch.int32, device=dev)
        self.grad_scale = 1.0
        self.param_names: list[str] | None = None  # (set_param_names: the keys of ema_state_dict)
        self.lr_schedule: LRSchedule | None = None
        self.ema_flat: torch.Tensor | None = None  # the parameters' moving average (set_ema), or None: off
        self.ema_decay = 0.0

    def set_ema(self, decay: float | None) -> None:
        """Keep an exponential moving average of the parameters, ``e <- e + (1 - decay) * (p - e)`` in fp32
        after every step, started at a copy of the current parameters (``ema_flat``); None switches it off
        and frees the buffer.  CPU parameters only: csed::sgd_flat has no average yet (the fused engine's
        update kernel has), and a GPU optimizer raises instead of averaging with torch kernels."""
        if decay is None:
            self.ema_flat, self.ema_decay = None, 0.0
            return
        if self.on_gpu:
            raise NotImplementedError("FusedSGD keeps a moving average on CPU parameters only: csed::sgd_flat "
                                      "does not update one (use the fused engine's set_ema on a GPU)")
        if not 0.0 <= float(decay) < 1.0:
            raise ValueError(f"ema decay {decay}: expected 0 <= decay < 1")
        self.ema_flat, self.ema_decay = self.flat.data.detach().clone(), float(decay)

    def set_lr_schedule(self, schedule: LRSchedule | None) -> None:
        """Train at ``schedule``'s rates from its current position (moved to the parameters' device) instead
        of ``param_groups[0]["lr"]``; None returns to the param group's value.  On the GPU the kernel
        reads the table entry of its step and advances the position itself, so a captured step serves
        the whole schedule."""
        self.lr_schedule = None if schedule is None else schedule.to(self.flat.device)

    def set_param_names(self, names) -> None:
        """The parameters' names in the optimizer's order (``[n for n, _ in model.named_parameters()]``)."""
        names = list(names)
        if len(names) != len(self.flat.params):
            raise ValueError("one name per parameter")
        self.param_names = names

    @property
    def on_gpu(self) -> bool:
        return self.flat.device.type == "cuda"

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
        if self.on_gpu:
            sch = self.lr_schedule
            _native.ops().sgd_flat(self.flat.data, self.flat.grad, self.momentum_flat, float(g["lr"]),
                                   float(g["momentum"]), float(g["dampening"]), float(g["weight_decay"]),
                                   bool(g["nesterov"]), float(self.grad_scale), self.step_count, self._ticket,
                                   None if sch is None else sch.table, None if sch is None else sch.pos)
        else:
            self._cpu_step(g)
        return loss

    def _cpu_step(self, g) -> None:
        lr, m, damp, wd, nest = g["lr"], g["momentum"], g["dampening"], g["weight_decay"], g["nesterov"]
        if self.lr_schedule is not None:
            lr = self.lr_schedule.current_lr()
            self.lr_schedule.pos += 1
        first = int(self.step_count.item()) == 0
        p, d, buf = self.flat.data, self.flat.grad * self.grad_scale, self.momentum_flat
        if wd:
            d = d + wd * p
        if m:
            if first:
                buf.copy_(d)
            else:
                buf.mul_(m).add_(d, alpha=1 - damp)
            d = d + m * buf if nest else buf
        p.add_(d, alpha=-lr)
        if self.ema_flat is not None:  # (1 - decay formed in fp32 from the fp32 decay, as the kernels form it)
            w = (torch.ones((), dtype=torch.float32) - torch.tensor(self.ema_decay, dtype=torch.float32)).item()
            self.ema_flat.add_(p - self.ema_flat, alpha=w)
        self.step_count += 1

    # ---- torch.optim.SGD-compatible state dict -------------------------------------------------
    def state_dict(self):
        if int(self.step_count.item()) > 0 and self.param_groups[0]["momentum"] != 0:
            for i, p in enumerate(self.flat.params):
                self.state[p]["momentum_buffer"] = self.flat.view(self.momentum_flat, i).detach().clone()
        sd = super().state_dict()
        if self.lr_schedule is not None:  # (what a torch scheduler leaves in the param group)
            sd["param_groups"][0]["lr"] = self.lr_schedule.current_lr()
        return sd

    def ema_state_dict(self) -> dict:
        """The averaged parameters under the model's parameter names where the optimizer was given them
        (``set_param_names``; else their indices): loads into the same module with ``load_state_dict``."""
        if self.ema_flat is None:
            raise RuntimeError("no moving average is kept (set_ema)")
        names = self.param_names or [str(i) for i in range(len(self.flat.params))]
        return {n: self.flat.view(self.ema_flat, i).detach().cpu().clone() for i, n in enumerate(names)}

    def load_ema_state_dict(self, sd: dict) -> None:
        """Restore ``ema_state_dict()``'s values (EMA must be on: the decay is not part of the file)."""
        if self.ema_flat is None:
            raise RuntimeError("no moving average is kept (set_ema)")
        names = self.param_names or [str(i) for i in range(len(self.flat.params))]
        with torch.no_grad():
            for i, n in enumerate(names):
                self.flat.view(self.ema_flat, i).copy_(sd[n])

    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        have = False
        with torch.no_grad():
            for i, p in enumerate(self.flat.params):
                st = self.state.get(p, {})
                mb = st.get("momentum_buffer")
                if mb is not None:
                    self.flat.view(self.momentum_flat, i).copy_(mb)
                    have = True
        self.step_count.fill_(1 if have else 0)
