"""Per-epoch random affine augmentation (shift / rotate / scale) of the device-resident train set.

The engines gather raw uint8 rows inside their kernels, so there is no place for a per-sample
host transform.  Instead ``AffineAugment.apply`` writes, once per epoch, an augmented uint8 copy
of the rows the epoch reads (``csed::augment_affine``, csrc/kernels/augment.hip) and the engines
read that copy.  The map of a row is a pure function of (seed, epoch, dataset row), so every rank
of a data-parallel run, and a resumed run, sees the images an uninterrupted single run would.

Definition (docs/ARCHITECTURE.md "Affine augmentation").  With c = 13.5 and
theta = (a, b, e, cc, d, f), output pixel (x, y) samples the source bilinearly at
``sx = a (x - c) + b (y - c) + c + e``, ``sy = cc (x - c) + d (y - c) + c + f``; taps outside the
image contribute 0; the byte is ``min(255, floor(v + 0.5))``.  Row r draws
``u_j = philox_uniform(seed, epoch, 4 r + j)`` and uses dx = (2 u0 - 1) max_shift, dy likewise from u1,
phi = (2 u2 - 1) max_rot_deg pi / 180, s = 1 + (2 u3 - 1) max_scale, a = d = cos(phi) / s,
b = -cc = sin(phi) / s, e = -dx, f = -dy.
"""
from __future__ import annotations

import math

import torch

from ..ops.rng import philox_uniform_reference


class AffineAugment:
    def __init__(self, max_shift: float = 0.0, max_rot_deg: float = 0.0, max_scale: float = 0.0,
                 seed: int | None = None):
        if not (max_shift >= 0 and max_rot_deg >= 0 and 0 <= max_scale < 1):
            raise ValueError(f"augmentation maxima shift {max_shift} px, rotation {max_rot_deg} deg, scale "
                             f"{max_scale}: expected shift >= 0, rotation >= 0 and 0 <= scale < 1")
        self.max_shift, self.max_rot_deg, self.max_scale = float(max_shift), float(max_rot_deg), float(max_scale)
        self._seed = None if seed is None else int(seed) & 0xFFFFFFFFFFFF
        self.epoch = 0  # which epoch's maps apply() draws; its callers advance it once per epoch

    @property
    def seed(self) -> int:
        if self._seed is None:  # follow torch.manual_seed(), as ops.rng.PhiloxState does
            self._seed = torch.initial_seed() & 0xFFFFFFFFFFFF
        return self._seed

    @property
    def enabled(self) -> bool:
        return self.max_shift > 0 or self.max_rot_deg > 0 or self.max_scale > 0

    def draw(self, rows: torch.Tensor) -> torch.Tensor:
        """The float32 [M, 6] maps of dataset rows ``rows`` at the current epoch, on the host (the CPU path's;
        the kernel draws its own, equal to rounding)."""
        import numpy as np

        r = rows.detach().cpu().numpy().astype(np.uint64)
        u = [philox_uniform_reference(self.seed, self.epoch, np.uint64(4) * r + np.uint64(j)) for j in range(4)]
        t = [torch.from_numpy(2.0 * v - 1.0) for v in u]  # float64 of the float32 draws
        phi = t[2] * (self.max_rot_deg * math.pi / 180.0)
        s = 1.0 + t[3] * self.max_scale
        a, b = torch.cos(phi) / s, torch.sin(phi) / s
        return torch.stack([a, b, -t[0] * self.max_shift, -b, a, -t[1] * self.max_shift], 1).to(torch.float32)

    def apply(self, src: torch.Tensor, dst: torch.Tensor, idx: torch.Tensor | None = None,
              theta: torch.Tensor | None = None, return_theta: bool = False) -> torch.Tensor | None:
        """Warp rows ``idx`` (int64; None: all) of the uint8 set ``src`` into the same rows of ``dst``, each by
        its own map drawn at ``self.epoch`` -- or by ``theta`` (float32 [M, 6], one inverse map per entry of
        ``idx``), which makes this a plain warp.  Rows not named keep what ``dst`` held.  ``return_theta``: the
        float32 maps used.  On a GPU this is one launch of ``csed::augment_affine``; on the CPU the same
        definition in float64 torch ops (the plumbing path of ``--device cpu``)."""
        if src.device.type == "cuda":
            from ..ops import _native

            M = src.shape[0] if idx is None else idx.numel()
            out = torch.empty((M, 6), dtype=torch.float32, device=src.device) if return_theta else None
            _native.ops().augment_affine(src, dst, idx, theta, out, self.seed, self.epoch, self.max_shift,
                                         self.max_rot_deg, self.max_scale)
            return out
        rows = torch.arange(src.shape[0]) if idx is None else idx.to(torch.long)
        theta = self.draw(rows) if theta is None else theta.to(torch.float32)
        dst.view(-1, 784)[rows] = _warp_cpu(src.view(-1, 784)[rows], theta)
        return theta if return_theta else None


def _warp_cpu(img: torch.Tensor, theta: torch.Tensor) -> torch.Tensor:
    """uint8 [M, 784] warped by float32 [M, 6] inverse maps, in float64."""
    M, c = img.shape[0], 13.5
    th = theta.to(torch.float64).view(M, 6, 1)
    p = torch.arange(784)
    x, y = (p % 28).to(torch.float64) - c, (p // 28).to(torch.float64) - c
    sx = th[:, 0] * x + th[:, 1] * y + c + th[:, 2]
    sy = th[:, 3] * x + th[:, 4] * y + c + th[:, 5]
    pad = torch.zeros((M, 31, 31), dtype=torch.float64)  # cells -1 .. 29: a zero border, as in the kernel
    pad[:, 1:29, 1:29] = img.view(M, 28, 28).to(torch.float64)
    sx, sy = sx.clamp(-1.0, 28.0), sy.clamp(-1.0, 28.0)
    x0, y0 = sx.floor(), sy.floor()
    fx, fy = sx - x0, sy - y0
    cell = ((y0 + 1) * 31 + (x0 + 1)).to(torch.long)
    flat = pad.view(M, -1)
    v00, v01 = flat.gather(1, cell), flat.gather(1, cell + 1)
    v10, v11 = flat.gather(1, cell + 31), flat.gather(1, cell + 32)
    v = (1 - fy) * ((1 - fx) * v00 + fx * v01) + fy * ((1 - fx) * v10 + fx * v11)
    return (v + 0.5).floor().clamp_(max=255).to(torch.uint8)
