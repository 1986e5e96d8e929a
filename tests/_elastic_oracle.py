"""The elastic augmentation's definition (docs/ARCHITECTURE.md "Elastic augmentation") in NumPy float64."""
import numpy as np

from csed_514_project_distributed_training_using_pytorch_amd.ops.rng import philox_uniform_reference

C = 13.5


def gauss(sigma):
    """The definition's G: float32 [32, 32], built in float64, one normalisation Z for every row, zero padding."""
    d = np.arange(-27.0, 28.0)
    i = np.arange(28.0)
    g = np.zeros((32, 32), dtype=np.float32)
    g[:28, :28] = np.exp(-(i[:, None] - i[None, :]) ** 2 / (2 * sigma ** 2)) / np.exp(-d * d / (2 * sigma ** 2)).sum()
    return g


def draw_disp(rows, seed, epoch, alpha, g):
    """float64 [M, 2, 28, 28] fields alpha (G U G) of dataset rows ``rows``, from the float32 G and draws."""
    at = 2 ** 40 + 1568 * np.asarray(rows, dtype=np.uint64)[:, None] + np.arange(1568, dtype=np.uint64)
    u = (2.0 * philox_uniform_reference(seed, epoch, at) - 1.0).reshape(-1, 2, 28, 28)
    g = g[:28, :28].astype(np.float64)
    return alpha * (g @ u @ g)


def warp_value(img, theta, disp):
    """The value v before rounding, float64 [M, 784]: ``img`` sampled at the affine coordinate plus ``disp``."""
    M = img.shape[0]
    th = np.asarray(theta, dtype=np.float64).reshape(M, 6, 1)
    d = np.asarray(disp, dtype=np.float64).reshape(M, 2, 784)
    p = np.arange(784)
    x, y = p % 28 - C, p // 28 - C
    sx = np.clip(th[:, 0] * x + th[:, 1] * y + C + th[:, 2] + d[:, 0], -1, 28)
    sy = np.clip(th[:, 3] * x + th[:, 4] * y + C + th[:, 5] + d[:, 1], -1, 28)
    x0, y0 = np.floor(sx), np.floor(sy)
    pad = np.zeros((M, 31, 31))  # cells -1 .. 29: taps outside the image are zeros
    pad[:, 1:29, 1:29] = img.reshape(M, 28, 28)
    v = np.zeros((M, 784))
    for dy, wy in ((0, 1 - (sy - y0)), (1, sy - y0)):
        for dx, wx in ((0, 1 - (sx - x0)), (1, sx - x0)):
            cell = ((y0 + dy + 1) * 31 + x0 + dx + 1).astype(np.int64)
            v += wy * wx * np.take_along_axis(pad.reshape(M, -1), cell, 1)
    return v


def warp(img, theta, disp):
    return np.minimum(255, np.floor(warp_value(img, theta, disp) + 0.5)).astype(np.uint8)
