"""The stroke augmentation's definition (docs/ARCHITECTURE.md "Stroke augmentation") in NumPy integers and plain
loops, and the cases tests/test_stroke_gpu.py and tests/test_stroke_cpu.py share."""
import numpy as np

from csed_514_project_distributed_training_using_pytorch_amd.ops.rng import philox_uniform_reference

SPANS = {0: (0,), 1: (1, 0), 2: (2, 1, 0), 3: (3, 2, 2, 0)}  # w_k(|dy|)
QS = (0, 1, 255, 256, 300, 512, 767, 768, 5000, -1, -256, -300, -768)
RECTS = {"all": (1, 0, 0, 28, 28), "last": (1, 27, 27, 1, 1), "clips": (1, -3, 20, 40, 40), "off": (0, 5, 5, 9, 9)}
SENTINEL = 0xAA
DRAWN = (2.5, 0.5, 4, 12)  # max_thickness, erase_p, erase_lo, erase_hi of the drawn cases


def rows():
    """uint8 [5, 784]: single 255 pixels at (x, y) = (0, 0), (27, 27), (13, 14), an all-255 row, a random row."""
    img = np.zeros((5, 28, 28), dtype=np.uint8)
    img[0, 0, 0] = img[1, 27, 27] = img[2, 14, 13] = 255
    img[3], img[4] = 255, np.random.default_rng(11).integers(0, 256, (28, 28), dtype=np.uint8)
    return img.reshape(5, 784)


EXPLICIT = {f"q{q}": (rows(), [(q, 0, 0, 0, 0, 0)] * 5) for q in QS}
EXPLICIT.update({f"{name}-q{q}": (rows()[4:], [(q, *rect)]) for q in (0, 300) for name, rect in RECTS.items()})


def extreme(img, k, neg):
    """M_k of one [28, 28] image: max (min if ``neg``) over the disc; taps outside the image read 0."""
    pad = np.pad(img.astype(np.int64), 3)
    taps = [pad[3 + dy:31 + dy, 3 + dx:31 + dx]  # one shifted copy of the image per pixel of the disc
            for dy in range(-k, k + 1) for dx in range(-SPANS[k][abs(dy)], SPANS[k][abs(dy)] + 1)]
    return np.minimum.reduce(taps) if neg else np.maximum.reduce(taps)


def apply(img, params):
    """(bytes, parameters used) of uint8 [M, 784] under int [M, 6] parameters (q, e, top, left, h, w)."""
    used, out = np.array(params, dtype=np.int32).reshape(-1, 6), np.empty_like(img)
    used[:, 0] = np.clip(used[:, 0], -768, 768)
    for i, (q, e, top, left, h, w) in enumerate(used.tolist()):
        k, p, I = abs(q) >> 8, abs(q) & 255, img[i].reshape(28, 28)
        v = (extreme(I, k, q < 0) * (256 - p) + extreme(I, min(k + 1, 3), q < 0) * p + 128) >> 8
        if e:
            v[max(top, 0):max(min(top + h, 28), 0), max(left, 0):max(min(left + w, 28), 0)] = 0
        out[i] = v.reshape(784)
    return out, used


def draw(rows_, seed, epoch, T, erase_p, lo, hi):
    out = []
    for r in rows_:
        at = np.uint64((1 << 41) + 8 * int(r)) + np.arange(6, dtype=np.uint64)
        u = philox_uniform_reference(seed, epoch, at).astype(np.float32)
        U = [int(v * 16777216.0) for v in u.astype(np.float64)]
        t = np.float32(np.float32(2.0 * float(u[0]) - 1.0) * np.float32(T))
        q = int(np.sign(t)) * int(np.floor(abs(float(t)) * 256.0))
        h, w = lo + ((U[2] * (hi - lo + 1)) >> 24), lo + ((U[3] * (hi - lo + 1)) >> 24)
        out.append((q, int(u[1] < np.float32(erase_p)), (U[4] * (29 - h)) >> 24, (U[5] * (29 - w)) >> 24, h, w))
    return np.array(out, dtype=np.int32)
