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

``ElasticAugment`` adds a per-row smoothed random displacement field to the sampling coordinate
(``csed::augment_elastic``, csrc/kernels/augment_elastic.hip) behind the same interface.

``StrokeAugment`` changes what no coordinate map can: stroke thickness (grey-level dilation / erosion by a disc) and
occlusion (a random rectangle set to 0), in integer arithmetic (``csed::augment_stroke``,
csrc/kernels/augment_stroke.hip).  It wraps one of the other two, or stands alone.
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


ELASTIC_STREAM = 1 << 40  # first Philox index of the raw displacement fields (the affine draws end below 2^33)


def gauss_table(sigma: float) -> torch.Tensor:
    """The definition's G: float32 [32, 32], the 28 x 28 matrix exp(-(i - k)^2 / (2 sigma^2)) / Z inside zero
    padding, Z the sum over d = -27 .. 27 (one normalisation for every row), built in float64."""
    import numpy as np

    d = np.arange(-27, 28, dtype=np.float64)
    z = np.exp(-d * d / (2.0 * sigma * sigma)).sum()
    i = np.arange(28, dtype=np.float64)
    g = np.zeros((32, 32), dtype=np.float32)
    g[:28, :28] = np.exp(-(i[:, None] - i[None, :]) ** 2 / (2.0 * sigma * sigma)) / z
    return torch.from_numpy(g)


class ElasticAugment(AffineAugment):
    """Elastic deformation (Simard, Steinkraus, Platt 2003) on top of the affine map: every row gets its own
    random displacement field, smoothed by a Gaussian of ``sigma`` pixels and scaled by ``alpha`` pixels
    (docs/ARCHITECTURE.md "Elastic augmentation").  With ``U_c[i][j] = 2 philox_uniform(seed, epoch,
    2^40 + 1568 r + 784 c + 28 i + j) - 1`` (c = 0: x, c = 1: y; i = pixel row) the field is
    ``D_c = alpha (G U_c G)`` and pixel (x, y) samples at the affine coordinate plus ``(D_0[y][x], D_1[y][x])``.
    ``alpha == 0`` is ``AffineAugment``, launch for launch."""

    CPU_CHUNK = 512  # rows per pass of the CPU path (1,568 float64 Philox draws per row)

    def __init__(self, alpha: float, sigma: float = 4.0, max_shift: float = 0.0, max_rot_deg: float = 0.0,
                 max_scale: float = 0.0, seed: int | None = None):
        super().__init__(max_shift, max_rot_deg, max_scale, seed)
        alpha, sigma = float(alpha), float(sigma)
        if not (math.isfinite(alpha) and alpha >= 0 and math.isfinite(sigma) and sigma > 0):
            raise ValueError(f"elastic augmentation alpha {alpha} px, sigma {sigma} px: expected a finite "
                             f"alpha >= 0 and a finite sigma > 0")
        self.alpha, self.sigma = alpha, sigma
        self._gauss: dict[torch.device, torch.Tensor] = {}

    @property
    def enabled(self) -> bool:
        return self.alpha > 0 or super().enabled

    def gauss(self, device) -> torch.Tensor:
        """The float32 [32, 32] table G on ``device`` (built once per device)."""
        device = torch.device(device)
        if device not in self._gauss:
            self._gauss[device] = gauss_table(self.sigma).to(device)
        return self._gauss[device]

    def draw_disp(self, rows: torch.Tensor) -> torch.Tensor:
        """The float32 [M, 2, 28, 28] fields of dataset rows ``rows`` at the current epoch, on the host in
        float64 (the CPU path's; the kernel draws the same U and smooths it in fp32 on the matrix cores)."""
        import numpy as np

        r = rows.detach().cpu().numpy().astype(np.uint64)
        at = np.uint64(ELASTIC_STREAM) + np.uint64(1568) * r[:, None] + np.arange(1568, dtype=np.uint64)
        u = torch.from_numpy(2.0 * philox_uniform_reference(self.seed, self.epoch, at) - 1.0).view(-1, 2, 28, 28)
        g = self.gauss("cpu")[:28, :28].to(torch.float64)
        return (self.alpha * (g @ u @ g)).to(torch.float32)

    def apply(self, src: torch.Tensor, dst: torch.Tensor, idx: torch.Tensor | None = None,
              theta: torch.Tensor | None = None, disp: torch.Tensor | None = None, return_theta: bool = False,
              return_disp: bool = False):
        """``AffineAugment.apply`` with the displacement field: drawn at ``self.epoch``, or ``disp`` (float32
        [M, 2, 28, 28], one field pair per entry of ``idx``: a plain flow-field warp).  Returns the float32 maps
        (``return_theta``), the float32 fields used (``return_disp``), both as a pair, or None.  On a GPU one
        launch of ``csed::augment_elastic``; on the CPU the definition in float64 torch ops."""
        if self.alpha == 0 and disp is None and not return_disp:
            return super().apply(src, dst, idx, theta, return_theta)
        M = src.shape[0] if idx is None else idx.numel()
        if src.device.type == "cuda":
            from ..ops import _native

            tout = torch.empty((M, 6), dtype=torch.float32, device=src.device) if return_theta else None
            dout = torch.empty((M, 2, 28, 28), dtype=torch.float32, device=src.device) if return_disp else None
            _native.ops().augment_elastic(src, dst, idx, theta, tout, disp, dout, self.gauss(src.device), self.seed,
                                          self.epoch, self.max_shift, self.max_rot_deg, self.max_scale, self.alpha)
        else:
            rows = torch.arange(src.shape[0]) if idx is None else idx.to(torch.long)
            tout = self.draw(rows) if theta is None else theta.to(torch.float32)
            dout = torch.empty((M, 2, 28, 28), dtype=torch.float32)
            for s in range(0, M, self.CPU_CHUNK):
                c = slice(s, s + self.CPU_CHUNK)
                dout[c] = self.draw_disp(rows[c]) if disp is None else disp[c].to(torch.float32)
                dst.view(-1, 784)[rows[c]] = _warp_cpu(src.view(-1, 784)[rows[c]], tout[c], dout[c])
        out = tuple(t for t, want in ((tout, return_theta), (dout, return_disp)) if want)
        return None if not out else out[0] if len(out) == 1 else out


def _warp_cpu(img: torch.Tensor, theta: torch.Tensor, disp: torch.Tensor | None = None) -> torch.Tensor:
    """uint8 [M, 784] warped by float32 [M, 6] inverse maps (plus float32 [M, 2, 28, 28] displacements), in
    float64."""
    M, c = img.shape[0], 13.5
    th = theta.to(torch.float64).view(M, 6, 1)
    p = torch.arange(784)
    x, y = (p % 28).to(torch.float64) - c, (p // 28).to(torch.float64) - c
    sx = th[:, 0] * x + th[:, 1] * y + c + th[:, 2]
    sy = th[:, 3] * x + th[:, 4] * y + c + th[:, 5]
    if disp is not None:
        d = disp.to(torch.float64).view(M, 2, 784)
        sx, sy = sx + d[:, 0], sy + d[:, 1]
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


STROKE_STREAM = 1 << 41  # first Philox index of the stroke draws (the elastic fields end well below it)
STROKE_SPANS = ((0,), (1, 0), (2, 1, 0), (3, 2, 2, 0))  # w_k(|dy|): the discs dx^2 + dy^2 <= k^2 as row half-widths


class StrokeAugment:
    """Stroke thickness and random erasing (docs/ARCHITECTURE.md "Stroke augmentation"), optionally after an
    ``AffineAugment`` / ``ElasticAugment`` (``inner``): every row is dilated or eroded by a disc of a random signed
    radius of up to ``max_thickness`` pixels (0 .. 3, in 1/256 px, two neighbouring integer discs blended), and with
    probability ``erase_p`` a random rectangle with sides in ``erase_size`` = (lo, hi) is set to 0.  All of it is
    integer arithmetic on the bytes: ``csed::augment_stroke`` (csrc/kernels/augment_stroke.hip) and the CPU path
    agree bit for bit.  The parameters (q, e, top, left, h, w) of a row are a pure function of (seed, epoch, dataset
    row); ``seed`` and ``epoch`` are shared with ``inner``.  With its own part off the augmenter is ``inner``, launch
    for launch."""

    CPU_CHUNK = 4096  # rows per pass of the CPU path

    def __init__(self, max_thickness: float = 0.0, erase_p: float = 0.0, erase_size: tuple[int, int] = (4, 12),
                 inner: AffineAugment | None = None, seed: int | None = None):
        max_thickness, erase_p = float(max_thickness), float(erase_p)
        lo, hi = (int(v) if float(v).is_integer() else -1 for v in map(float, erase_size))  # (NaN, 4.5: rejected)
        if not (0 <= max_thickness <= 3 and 0 <= erase_p <= 1 and 1 <= lo <= hi <= 28):
            raise ValueError(f"stroke augmentation thickness {max_thickness} px, erase probability {erase_p}, erase "
                             f"size {tuple(erase_size)}: expected 0 <= thickness <= 3, 0 <= probability <= 1 and "
                             f"integer sides 1 <= lo <= hi <= 28")
        self.max_thickness, self.erase_p, self.erase_size, self.inner = max_thickness, erase_p, (lo, hi), inner
        self._seed = None if seed is None else int(seed) & 0xFFFFFFFFFFFF
        if inner is not None and seed is not None:
            inner._seed = self._seed
        self.epoch = 0 if inner is None else inner.epoch

    @property
    def seed(self) -> int:
        if self._seed is None:  # inner's, which follows torch.manual_seed() as AffineAugment's does
            self._seed = self.inner.seed if self.inner is not None else torch.initial_seed() & 0xFFFFFFFFFFFF
        return self._seed

    @property
    def epoch(self) -> int:
        return self._epoch

    @epoch.setter
    def epoch(self, value: int) -> None:  # (the engines do ``augment.epoch += 1``; inner draws at the same epoch)
        self._epoch = value
        if self.inner is not None:
            self.inner.epoch = value

    @property
    def own(self) -> bool:
        return self.max_thickness > 0 or self.erase_p > 0

    @property
    def enabled(self) -> bool:
        return self.own or (self.inner is not None and self.inner.enabled)

    def draw(self, rows: torch.Tensor) -> torch.Tensor:
        """The int32 [M, 6] parameters (q, e, top, left, h, w) of dataset rows ``rows`` at the current epoch, on the
        host: the kernel's own draw, value for value."""
        import numpy as np

        r = rows.detach().cpu().numpy().astype(np.uint64)
        u = [philox_uniform_reference(self.seed, self.epoch, np.uint64(STROKE_STREAM) + np.uint64(8) * r + np.uint64(j))
             .astype(np.float32) for j in range(6)]  # (multiples of 2^-24: exact in float32)
        U = [(v.astype(np.float64) * 16777216.0).astype(np.int64) for v in u]
        t = (np.float32(2) * u[0] - np.float32(1)) * np.float32(self.max_thickness)  # float32, one rounding
        q = np.sign(t).astype(np.int64) * np.floor(np.abs(t) * np.float32(256)).astype(np.int64)
        lo, hi = self.erase_size
        n = hi - lo + 1
        h, w = lo + ((U[2] * n) >> 24), lo + ((U[3] * n) >> 24)
        cols = [q, u[1] < np.float32(self.erase_p), (U[4] * (29 - h)) >> 24, (U[5] * (29 - w)) >> 24, h, w]
        return torch.from_numpy(np.stack([c.astype(np.int32) for c in cols], 1))

    def apply(self, src: torch.Tensor, dst: torch.Tensor, idx: torch.Tensor | None = None,
              params: torch.Tensor | None = None, return_params: bool = False) -> torch.Tensor | None:
        """Rows ``idx`` (int64; None: all) of the uint8 set ``src`` into the same rows of ``dst``: first through
        ``inner`` (if enabled), then thickened / thinned and erased by each row's parameters drawn at ``self.epoch``
        -- or by ``params`` (int32 [M, 6], one entry per entry of ``idx``), a plain morphology + mask.
        ``return_params``: the int32 parameters used.  ``dst`` may be ``src``; the entries of ``idx`` must then be
        distinct (an epoch order's are), since a row named twice would be processed twice.  On a GPU this is one
        launch of ``csed::augment_stroke`` (after inner's, in place on ``dst``); on the CPU the same definition in
        integer torch ops (the plumbing path of ``--device cpu``)."""
        inner = self.inner if self.inner is not None and self.inner.enabled else None
        if inner is not None:
            if not self.own and params is None and not return_params:
                return inner.apply(src, dst, idx)
            inner.apply(src, dst, idx)
            src = dst
        lo, hi = self.erase_size
        if src.device.type == "cuda":
            from ..ops import _native

            M = src.shape[0] if idx is None else idx.numel()
            out = torch.empty((M, 6), dtype=torch.int32, device=src.device) if return_params else None
            _native.ops().augment_stroke(src, dst, idx, params, out, self.seed, self.epoch, self.max_thickness,
                                         self.erase_p, lo, hi)
            return out
        rows = torch.arange(src.shape[0]) if idx is None else idx.to(torch.long)
        params = self.draw(rows) if params is None else params.to(torch.int32).clone()
        params[:, 0].clamp_(-768, 768)
        for s in range(0, rows.numel(), self.CPU_CHUNK):
            c = rows[s:s + self.CPU_CHUNK]
            dst.view(-1, 784)[c] = _stroke_cpu(src.view(-1, 784)[c], params[s:s + self.CPU_CHUNK])
        return params if return_params else None


def _stroke_cpu(img: torch.Tensor, params: torch.Tensor) -> torch.Tensor:
    """uint8 [M, 784] through the stroke definition with int32 [M, 6] parameters (q already clamped).  Erosion runs
    as dilation of the complemented image inside a border of 255, i.e. of zeros before the complement."""
    M = img.shape[0]
    P = params.to(torch.int64).view(M, 6, 1, 1)
    q, e, top, left, h, w = (P[:, j] for j in range(6))
    a, neg = q.abs(), q < 0
    k, p = a >> 8, a & 255
    k1 = (k + 1).clamp(max=3)
    I = img.view(M, 28, 28).to(torch.int64)
    I = torch.where(neg, 255 - I, I)
    pad = (neg * 255).expand(M, 34, 34).clone()
    pad[:, 3:31, 3:31] = I
    maxima = [I]  # M_0 .. M_3: shifted maxima over the discs' spans
    for spans in STROKE_SPANS[1:]:
        m = I
        for ady, half in enumerate(spans):
            for dy in {ady, -ady}:
                for dx in range(-half, half + 1):
                    m = torch.maximum(m, pad[:, 3 + dy:31 + dy, 3 + dx:31 + dx])
        maxima.append(m)
    S = torch.stack(maxima, 1)
    S = torch.where(neg.view(M, 1, 1, 1), 255 - S, S)
    at = torch.arange(M)
    v = (S[at, k.view(M)] * (256 - p) + S[at, k1.view(M)] * p + 128) >> 8
    y, x = torch.arange(28).view(1, 28, 1), torch.arange(28).view(1, 1, 28)
    erased = (e != 0) & (y >= top) & (y < top + h) & (x >= left) & (x < left + w)
    return v.masked_fill(erased, 0).to(torch.uint8).view(M, 784)
