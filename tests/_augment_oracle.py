"""The affine augmentation's definition (docs/ARCHITECTURE.md "Affine augmentation") in NumPy float64."""
import numpy as np

from csed_514_project_distributed_training_using_pytorch_amd.ops.rng import philox_uniform_reference

C = 13.5
# the exact cases: integer shifts (e, f), and the quarter turn that maps pixel centres to pixel centres
EXACT = {"identity": (1, 0, 0, 0, 1, 0), "right1": (1, 0, 1, 0, 1, 0), "left1": (1, 0, -1, 0, 1, 0),
         "down3": (1, 0, 0, 0, 1, 3), "up3": (1, 0, 0, 0, 1, -3), "corner": (1, 0, -27, 0, 1, 27),
         "gone": (1, 0, 28, 0, 1, 0), "turn90": (0, 1, 0, -1, 0, 0)}


def rows(n, seed=5):
    img = np.random.default_rng(seed).integers(0, 256, (n, 784), dtype=np.uint8)
    img[-1] = 255
    return img


def draw_theta(rows, seed, epoch, max_shift, max_rot_deg, max_scale):
    """float64 [M, 6] maps (a, b, e, cc, d, f) of dataset rows ``rows``, from the float32 draws."""
    rows = np.asarray(rows, dtype=np.uint64)
    t = [2.0 * philox_uniform_reference(seed, epoch, np.uint64(4) * rows + np.uint64(j)) - 1.0 for j in range(4)]
    phi = t[2] * max_rot_deg * np.pi / 180.0
    s = 1.0 + t[3] * max_scale
    a, b = np.cos(phi) / s, np.sin(phi) / s
    return np.stack([a, b, -t[0] * max_shift, -b, a, -t[1] * max_shift], 1)


def warp_value(img, theta):
    """The value v before rounding, float64 [M, 784], of uint8 [M, 784] ``img`` under [M, 6] ``theta``."""
    M = img.shape[0]
    th = np.asarray(theta, dtype=np.float64).reshape(M, 6, 1)
    p = np.arange(784)
    x, y = p % 28 - C, p // 28 - C
    sx = th[:, 0] * x + th[:, 1] * y + C + th[:, 2]
    sy = th[:, 3] * x + th[:, 4] * y + C + th[:, 5]
    x0, y0 = np.floor(sx), np.floor(sy)
    im = img.reshape(M, 784).astype(np.float64)
    v = np.zeros((M, 784))
    for dy, wy in ((0, 1 - (sy - y0)), (1, sy - y0)):
        for dx, wx in ((0, 1 - (sx - x0)), (1, sx - x0)):
            tx, ty = x0 + dx, y0 + dy
            inside = (tx >= 0) & (tx <= 27) & (ty >= 0) & (ty <= 27)
            cell = (np.clip(ty, 0, 27) * 28 + np.clip(tx, 0, 27)).astype(np.int64)
            v += np.where(inside, wy * wx * np.take_along_axis(im, cell, 1), 0.0)
    return v


def warp(img, theta):
    return np.minimum(255, np.floor(warp_value(img, theta) + 0.5)).astype(np.uint8)
