"""Oracle of csrc/kernels/elementwise.hip: log-softmax, NLL, their fusion, max-pool + ReLU, dropout, the channel
mask, the ReLU / dropout gate and the batch gather + normalise.  Host only: float64 torch / numpy and integers,
no GPU, none of the project's ops (ops/rng.py's NumPy Philox reference excepted).  Every function is written from
the operation's definition, not from the kernel's loops.  tests/test_elementwise_oracle_cpu.py ties each function
to torch's own float64 ops and asserts the preconditions of every exact case; tests/test_elementwise_oracle_gpu.py
runs the kernels against it.

What is exact and what carries a bound (u = 2^-24, one fp32 rounding):

  nll_fwd      exact.  Log-probs are integers in [-64, 0] and at most 600 rows: every partial sum of the serial
               and tree reduction is an integer below 2^24, so `none` and `sum` are bit-exact in any order; `mean`
               is one correctly rounded fp32 divide of two exact fp32 values (``div32``: the build passes no
               fast-math flag and hipcc keeps fp32 divide correctly rounded, see _adam_oracle.py).  `correct` is an
               integer count; the lowest index among equal maxima wins (the kernel's strict `>`).
  nll_bwd      exact.  -g, or one correctly rounded divide -(g / rows), and 0 elsewhere.
  maxpool_relu_fwd / _bwd   exact.  A maximum, a sign test and one product of small integers with a scale in
               {0, 1, 2}; the argmax byte is dy * k + dx of the first maximum in row-major window order, and of the
               last NaN if the window has one (torch's max_pool2d rule `v > best || isnan(v)`; the tests plant one
               NaN per window).  relu comes before the scale; H and W are floored.
  dropout_fwd / channel_mask   exact.  The keep decision is an integer Philox draw (a multiple of 2^-24) compared
               with the fp32 value of p; the scale is the correctly rounded fp32 1 / (1 - p) (0 at p >= 1, so
               nothing becomes inf or NaN); a kept value is one fp32 product rounded once to the output dtype.
  gate_bwd     exact.  One fp32 product (exact for s in {1, 2}), rounded once to dx's dtype; y > 0 decides, so
               0, -0.0, NaN and negatives gate to 0.
  gather_normalize   exact.  inv_std = 1 / fp32(std), scale = inv_std * fp32(1 / 255) and shift = -fp32(mean) *
               inv_std are formed in fp32 as the launcher and the kernel form them; byte * scale + shift needs at
               most 8 + 24 bits next to a 24-bit addend of a nearby exponent, which float64 holds exactly (the CPU
               test proves it against rationals for all 256 bytes), so the fused multiply-add is that value rounded
               once to fp32, then once to the output dtype.
  log_softmax_fwd, lsm_nll_fwd (log-probs and per-row losses)   bound, per element of row r:
                   C_FWD * u * max(1, max_c |x_rc| + |lse_r|)
               The kernels use __expf / __logf (v_exp_f32 / v_log_f32 around one fp32 multiply each).  Largest error
               measured on an MI355X over all cases of the GPU test, in these units: 1.647 (log_softmax_fwd) and
               1.749 (lsm_nll_fwd), MEASURED_FWD below; C_FWD = 8 is four times that (7.0), rounded up to a power of
               two: the margin covers other inputs and another, equally valid instruction choice by the compiler.  Planted -inf entries are asserted exactly.
  lsm_nll_fwd's reduced loss   the sum of its rows' bounds plus (ceil(rows / 256) + 8) * u * sum |v| for the
               serial-plus-tree fp32 sum (ceil(rows / 256) - 1 serial adds per thread, 8 tree levels, one spare
               for the divide), all divided by rows for `mean`.
  log_softmax_bwd   C_BWD * u * (|dy_rc| + |sum_c dy_rc|), then the store's rounding to dx's dtype.  dy is small
               integers (the sum is exact in any order); the error is __expf's and one fused multiply-add's.
  lsm_nll_bwd  C_BWD * u * |g_r| (g_r = g / rows for `mean`, its divide included), then the store's rounding.
               Both backward bounds are applied as an interval: the kernel's fp32 value f has |f - ref| <= b and
               rounding is monotone, so the stored value lies in [round(ref - b), round(ref + b)] -- never wider
               than b plus half an ulp of the output dtype.
               Largest measured error in these units: 1.022 (log_softmax_bwd) and 1.651 (lsm_nll_bwd),
               MEASURED_BWD below; C_BWD = 8 is chosen like C_FWD (4 x 1.651 = 6.6).
"""
from __future__ import annotations

import math
import os
import sys
from fractions import Fraction

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from _exact_oracle import DTYPES, F64, expected, ints, round_trips  # noqa: E402,F401

from csed_514_project_distributed_training_using_pytorch_amd.ops.rng import philox_uniform_reference  # noqa: E402

U = 2.0 ** -24
# Largest errors measured on an MI355X over every case of tests/test_elementwise_oracle_gpu.py, in the units of
# the bounds above, and the constants chosen from them (4 x measured, rounded up to a power of two).
MEASURED_FWD = 1.749  # log_softmax_fwd 1.647, lsm_nll_fwd 1.749
MEASURED_BWD = 1.651  # log_softmax_bwd 1.022, lsm_nll_bwd 1.651
C_FWD = 8.0  # 4 x 1.749 = 7.0
C_BWD = 8.0  # 4 x 1.651 = 6.6

RED = {"none": 0, "mean": 1, "sum": 2}


def dt_name(dtype) -> str:
    return {torch.bfloat16: "bf16", torch.float16: "f16", torch.float32: "f32"}[dtype]


def div32(a, b) -> np.float32:
    """One correctly rounded fp32 divide of two values that fp32 holds exactly."""
    a32, b32 = np.float32(a), np.float32(b)
    assert float(a32) == float(a) and float(b32) == float(b)
    return a32 / b32


# ------------------------------------------------------------- log-softmax / NLL
def lse_ref(x64: torch.Tensor) -> torch.Tensor:
    """log sum_c exp(x_rc), [rows, 1]"""
    x = x64.to(F64)
    m = x.max(1, keepdim=True).values
    return m + (x - m).exp().sum(1, keepdim=True).log()


def log_softmax_ref(x64: torch.Tensor) -> torch.Tensor:
    x = x64.to(F64)
    return x - lse_ref(x)


def log_softmax_bwd_ref(dy64: torch.Tensor, y64: torch.Tensor) -> torch.Tensor:
    """dy - exp(y) * sum_c dy"""
    dy, y = dy64.to(F64), y64.to(F64)
    return dy - y.exp() * dy.sum(1, keepdim=True)


def fwd_scale(x64: torch.Tensor) -> torch.Tensor:
    """max(1, max_c |x_rc| + |lse_r|), [rows, 1]; the maximum runs over the finite entries."""
    x = x64.to(F64)
    top = torch.where(x.isinf(), torch.zeros((), dtype=F64), x.abs()).max(1, keepdim=True).values
    return (top + lse_ref(x).abs()).clamp_min(1.0)


def fwd_bound(x64: torch.Tensor, c: float = None) -> torch.Tensor:
    """c * u * fwd_scale: the forward log-softmax kernels' bound per element of a row, [rows, 1]"""
    return (C_FWD if c is None else c) * U * fwd_scale(x64)


def nll_ref(logp64: torch.Tensor, target: torch.Tensor, reduction: str) -> torch.Tensor:
    v = -logp64.to(F64).gather(1, target.view(-1, 1)).squeeze(1)
    if reduction == "none":
        return v
    return v.sum() / v.shape[0] if reduction == "mean" else v.sum()


def correct_ref(logp: torch.Tensor, target: torch.Tensor) -> int:
    """Rows whose predicted class is the target; the prediction is the LOWEST index among equal maxima."""
    lp = logp.to(F64)
    cols = torch.arange(lp.shape[1]).view(1, -1).expand_as(lp)
    is_max = lp == lp.max(1, keepdim=True).values
    pred = torch.where(is_max, cols, torch.full_like(cols, lp.shape[1])).min(1).values
    return int((pred == target).sum())


def _row_grad(g64: torch.Tensor, rows: int, reduction: str) -> torch.Tensor:
    g = g64.to(F64).reshape(-1)
    if reduction == "none":
        return g.view(rows, 1)
    return (g / rows if reduction == "mean" else g).view(1, 1).expand(rows, 1)


def _onehot(target: torch.Tensor, C: int) -> torch.Tensor:
    return torch.zeros(target.shape[0], C, dtype=F64).scatter_(1, target.view(-1, 1), 1.0)


def nll_bwd_ref(g64: torch.Tensor, target: torch.Tensor, C: int, reduction: str) -> torch.Tensor:
    """-g_r at the target's class, 0 elsewhere (g_r = g / rows for mean)"""
    return -_row_grad(g64, target.shape[0], reduction) * _onehot(target, C)


def lsm_nll_ref(z64: torch.Tensor, target: torch.Tensor, reduction: str):
    """(log-probs, nll of them)"""
    logp = log_softmax_ref(z64)
    return logp, nll_ref(logp, target, reduction)


def lsm_nll_bwd_ref(g64: torch.Tensor, logp64: torch.Tensor, target: torch.Tensor, reduction: str) -> torch.Tensor:
    """g_r * (exp(logp) - onehot)"""
    lp = logp64.to(F64)
    return _row_grad(g64, lp.shape[0], reduction) * (lp.exp() - _onehot(target, lp.shape[1]))


# ------------------------------------------------------------------------ pool
def _windows(x: torch.Tensor, k: int) -> torch.Tensor:
    N, C, H, W = x.shape
    PH, PW = H // k, W // k
    return x[:, :, :PH * k, :PW * k].reshape(N, C, PH, k, PW, k).permute(0, 1, 2, 4, 3, 5).reshape(N, C, PH, PW, k * k)


def pool_fwd_ref(x: torch.Tensor, k: int, scale: torch.Tensor | None = None):
    """(relu(max of each k x k window) * scale[n * C + c], argmax byte dy * k + dx).  The first maximum in row-major
    window order wins; a window with a NaN gives NaN and names its last NaN; H and W are floored."""
    win = _windows(x.to(F64), k)
    best = win[..., 0].clone()
    idx = torch.zeros(win.shape[:-1], dtype=torch.uint8)
    for r in range(1, k * k):
        more = win[..., r] > best  # (strict: a tie keeps the earlier position)
        best = torch.where(more, win[..., r], best)
        idx = torch.where(more, torch.full_like(idx, r), idx)
    isn = win.isnan()
    has_nan = isn.any(-1)
    last_nan = (isn * torch.arange(k * k)).max(-1).values.to(torch.uint8)
    out = torch.where(has_nan, torch.full_like(best, float("nan")), best.clamp_min(0))
    idx = torch.where(has_nan, last_nan, idx)
    if scale is not None:
        out = out * scale.to(F64).view(x.shape[0], x.shape[1], 1, 1)
    return out, idx


def unpool_ref(dyp: torch.Tensor, idx: torch.Tensor, out: torch.Tensor, k: int, shape, scale=None) -> torch.Tensor:
    """maxpool_relu_bwd's rule for k x k windows on an input of ``shape``: the window position idx names gets
    dyp * scale where the pooled output is > 0; everything else, the floored-off border included, is 0.
    (_exact_oracle.unpool_ref is the k = 2, even-plane case; the CPU test ties the two.)"""
    N, C, H, W = shape
    PH, PW = H // k, W // k
    g = dyp.to(F64) * (out.to(F64) > 0)
    if scale is not None:
        g = g * scale.to(F64).view(N, C, 1, 1)
    win = torch.zeros(N, C, PH, PW, k * k, dtype=F64)
    win.scatter_(4, idx.long().unsqueeze(-1), g.unsqueeze(-1))
    dx = torch.zeros(N, C, H, W, dtype=F64)
    dx[:, :, :PH * k, :PW * k] = win.view(N, C, PH, PW, k, k).permute(0, 1, 2, 4, 3, 5).reshape(N, C, PH * k, PW * k)
    return dx


# --------------------------------------------------------------------- dropout
def keep_ref(seed: int, offset: int, offset_dev: int | None, idx, p: float) -> np.ndarray:
    """Element idx of stream (seed, offset + (offset_dev << 20)) is kept: its draw is >= the fp32 value of p."""
    off = int(offset) + ((int(offset_dev) << 20) if offset_dev is not None else 0)
    return philox_uniform_reference(int(seed), off, idx) >= np.float32(p)


def dropout_scale(p: float) -> np.float32:
    p32 = np.float32(p)
    return np.float32(0) if p32 >= np.float32(1) else np.float32(1) / (np.float32(1) - p32)


def _times32(x: torch.Tensor, s) -> torch.Tensor:
    """fp32(x) * fp32(s): one fp32 product"""
    return x.to(torch.float32) * torch.tensor(float(np.float32(s)), dtype=torch.float32)


def dropout_ref(x: torch.Tensor, inner: int, p: float, seed: int, offset: int, offset_dev: int | None):
    """(y, keep): element i belongs to Philox element i // inner in channel mode (inner > 0), i otherwise; a kept
    value is fp32(x) * scale rounded once to x's dtype."""
    n = x.numel()
    e = np.arange(n) // inner if inner > 0 else np.arange(n)
    keep = torch.from_numpy(keep_ref(seed, offset, offset_dev, e, p)).view(x.shape)
    y = torch.where(keep, _times32(x, dropout_scale(p)).to(x.dtype), torch.zeros((), dtype=x.dtype))
    return y, keep


def channel_mask_ref(n: int, p: float, seed: int, offset: int, offset_dev: int | None) -> torch.Tensor:
    keep = torch.from_numpy(keep_ref(seed, offset, offset_dev, np.arange(n), p))
    return torch.where(keep, torch.tensor(float(dropout_scale(p)), dtype=torch.float32), torch.zeros((), dtype=torch.float32))


def gate_bwd_ref(dout: torch.Tensor, y: torch.Tensor, s: float) -> torch.Tensor:
    """fp32(dout) * fp32(s) rounded once to dout's dtype where y > 0, else 0 (so for y = 0, -0.0, NaN, negatives)"""
    return torch.where(y.to(F64) > 0, _times32(dout, s).to(dout.dtype), torch.zeros((), dtype=dout.dtype))


# ------------------------------------------------------------ gather_normalize
def normalize_constants(mean: float, std: float):
    """(scale, shift) in fp32, formed as launch_gather_normalize and the kernel form them"""
    inv_std = np.float32(1) / np.float32(std)
    return inv_std * (np.float32(1) / np.float32(255)), -np.float32(mean) * inv_std


def normalize_exact(byte: int, mean: float, std: float) -> Fraction:
    """byte * scale + shift as a rational number"""
    scale, shift = normalize_constants(mean, std)
    return Fraction(int(byte)) * Fraction(float(scale)) + Fraction(float(shift))


def gather_normalize_ref(src: torch.Tensor, idx: torch.Tensor, cursor: int | None, B: int, mean: float, std: float,
                         dtype: torch.dtype):
    """(images [B, elems] in ``dtype``, the B source rows taken): rows idx[cursor * B : cursor * B + B]; every
    byte through fma(byte, scale, shift), exact in float64, rounded once to fp32 and then to ``dtype``."""
    base = (0 if cursor is None else int(cursor)) * B
    rows = idx[base:base + B].long()
    scale, shift = normalize_constants(mean, std)
    v = src[rows].reshape(B, -1).to(F64) * float(scale) + float(shift)
    return expected(v, dtype), rows


# ----------------------------------------------------------------------- cases
# (here, so that the CPU test asserts their preconditions without a GPU)
LSM_ROWS = (1, 3, 4, 5, 9)
LSM_COLS = (1, 2, 10, 63, 64, 65, 130)
NLL_ROWS = (1, 2, 255, 256, 257, 600)
FUSED_ROWS = (1, 255, 256, 257, 600)
NLL_COLS = (1, 10, 33)
SHIFT = 80.0


def _gen(*key) -> torch.Generator:
    return torch.Generator().manual_seed(abs(hash(tuple(int(k) for k in key))) % (2 ** 31))


def logits(rows: int, C: int, dtype, kind: str = "randn"):
    """(x in ``dtype``, the float64 input whose log-softmax is expected).  randn: 3 * randn rounded to the dtype;
    up / down (fp32): multiples of 2^-10 shifted by +-80, exactly, so the answer is the unshifted one's; inf: some
    but not all entries of every row -inf (entry 0 stays finite)."""
    g = _gen(rows, C, 11)
    x = torch.randn(rows, C, generator=g, dtype=F64) * 3
    if kind in ("up", "down"):
        base = (x * 1024).round() / 1024
        return (base + (SHIFT if kind == "up" else -SHIFT)).to(dtype), base
    x = x.to(dtype)
    if kind == "inf":
        hole = torch.rand(rows, C, generator=g) < 0.4
        hole[:, 0] = False
        hole[:, C - 1] = True
        x = torch.where(hole, torch.full_like(x, float("-inf")), x)
    return x, x.to(F64)


def int_grads(rows: int, C: int) -> torch.Tensor:
    """dy of the log-softmax backward: integers in [-4, 4], so every row sum is exact in fp32 in any order"""
    return ints(_gen(rows, C, 12), (rows, C), -4, 4)


def targets(rows: int, C: int) -> torch.Tensor:
    return torch.randint(0, C, (rows,), generator=_gen(rows, C, 13))


def int_logp(rows: int, C: int):
    """(integer log-probs in [-64, 0], targets) with planted ties: in every third row the row maximum 0 stands at the
    target's class and at one other class, below it or above it in turn."""
    g = _gen(rows, C, 14)
    lp = ints(g, (rows, C), -64, -1)
    t = targets(rows, C)
    r = torch.arange(rows)
    tie = r % 3 == 0
    lp[r[tie], t[tie]] = 0.0
    if C > 1:
        other = (t + 1 + (r % (C - 1))) % C  # (never the target itself)
        lp[r[tie], other[tie]] = 0.0
        hit = r % 3 == 1  # (a row the target wins alone)
        lp[r[hit], t[hit]] = 0.0
    return lp, t


def int_gout(rows: int, reduction: str) -> torch.Tensor:
    n = rows if reduction == "none" else 1
    g = ints(_gen(rows, n, 15), (n,), -8, 8)
    g[0] = 3.0
    return g


POOL_SHAPES = [(2, (3, 5, 8, 12)), (2, (2, 3, 7, 9)), (3, (2, 3, 7, 10)), (2, (1, 2, 34, 34)), (2, (1, 1, 2, 2)),
               (2, (1, 1, 2, 514))]  # (the last: 257 pooled elements, one past a 256-thread block)
POOL_KINDS = ("ties", "negwin", "nanfirst", "nanmid", "nanlast", "negzero")


def pool_id(k: int, shape) -> str:
    PH, PW = shape[2] // k, shape[3] // k
    tag = {289: "-plane289", 1: "-onewindow"}.get(PH * PW, "")
    if shape[0] * shape[1] * PH * PW == 257:
        tag = "-total257"
    return f"k{k}-" + "x".join(map(str, shape)) + tag


def pool_input(k: int, shape, kind: str) -> torch.Tensor:
    """float64 small integers (exact in every dtype).  ties: values in [-2, 3], and about 30 % of the windows get
    their maximum copied to a second position; negwin: half the windows all negative; nanfirst / mid / last: one
    NaN at that position of every other window; negzero: values in {-0.0, 0.0, -1} so that zeros of both signs tie."""
    N, C, H, W = shape
    g = _gen(k, H, W, N, len(kind), ord(kind[3]))
    x = ints(g, shape, -2, 3)
    PH, PW = H // k, W // k
    n, c, ph, pw = torch.meshgrid(torch.arange(N), torch.arange(C), torch.arange(PH), torch.arange(PW), indexing="ij")
    wid = ((n * C + c) * PH + ph) * PW + pw

    def put(sel, pos, val):
        x[n[sel], c[sel], ph[sel] * k + pos[sel] // k, pw[sel] * k + pos[sel] % k] = val[sel] if torch.is_tensor(val) else val

    if kind == "ties":
        win = _windows(x, k)
        sel = torch.rand(wid.shape, generator=g) < 0.3
        pos = torch.randint(0, k * k, wid.shape, generator=g)
        put(sel, pos, win.max(-1).values)
    elif kind == "negwin":
        neg = (wid % 2 == 0).view(N, C, PH, 1, PW, 1).expand(N, C, PH, k, PW, k).reshape(N, C, PH * k, PW * k)
        x[:, :, :PH * k, :PW * k] = torch.where(neg, -x[:, :, :PH * k, :PW * k].abs() - 1, x[:, :, :PH * k, :PW * k])
    elif kind.startswith("nan"):
        at = {"nanfirst": 0, "nanmid": (k * k) // 2, "nanlast": k * k - 1}[kind]
        put(wid % 2 == 0, torch.full_like(wid, at), float("nan"))
    elif kind == "negzero":
        v = torch.randint(0, 3, shape, generator=g)
        x = torch.where(v == 0, torch.tensor(-0.0, dtype=F64), torch.where(v == 1, torch.tensor(0.0, dtype=F64),
                                                                           torch.tensor(-1.0, dtype=F64)))
    return x


def pool_scale(shape, which: str):
    if which == "noscale":
        return None
    return ints(_gen(shape[0], shape[1], 16), (shape[0] * shape[1],), 0, 1) * 2.0


DROP_PS = (0.0, 0.3, 0.5, 1.0)
DROP_OFFSETS = (0, 7)
DROP_DEVS = (None, 0, 3)
DROP_SEED = 0x5EED1234ABC
DROP_TOTALS = (1, 255, 256, 257, 4099)
DROP_INNERS = (1, 35, 64)
DROP_CHANNELS = 70
MASK_NS = (1, 256, 257, 1400)
GATE_NS = (1, 257)
GATE_SCALES = {"s1": 1.0, "s2": 2.0, "sinv0.7": float(np.float32(1 / 0.7))}


def p_id(p: float) -> str:
    return "p" + ("%g" % p)


def drop_input(n: int, dtype) -> torch.Tensor:
    """randn rounded to the dtype, no zeros (so y != 0 is the mask wherever the scale is not 0)"""
    x = torch.randn(n, generator=_gen(n, 17), dtype=F64)
    return torch.where(x.abs() < 0.01, torch.ones((), dtype=F64), x).to(dtype)


def gate_input(n: int, ddt, ydt, exact: bool):
    """(dout, y): dout small integers (exact cases) or randn, in ddt; y in ydt with 0, -0.0, NaN and negatives."""
    g = _gen(n, 18)
    dout = (ints(g, (n,), -4, 4) if exact else torch.randn(n, generator=g, dtype=F64)).to(ddt)
    y = torch.randn(n, generator=g, dtype=F64)
    if n > 8:
        y[1], y[2], y[3], y[4], y[n - 1] = 0.0, -0.0, float("nan"), -2.0, float("nan")
    y[0] = 1.5
    return dout, y.to(ydt)


GN_ROWS, GN_B = 11, 3
GN_IDX = (7, 2, 7, 10, 0, 3, 5, 5, 1, 9)
GN_MEAN, GN_STD = 0.1307, 0.3081
GN_ELEMS = (5, 784)
GN_CURSORS = (None, 0, 2)


def gather_input(elems: int):
    """(src uint8 [11, elems], idx, labels_src): at 784 elements every row holds all 256 byte values"""
    src = ((torch.arange(GN_ROWS * elems) * 37 + 255) % 256).to(torch.uint8).view(GN_ROWS, elems)
    if elems < 256:
        src[:, 0], src[:, 1] = 0, 255
    return src, torch.tensor(GN_IDX, dtype=torch.long), (torch.arange(GN_ROWS) * 3 + 1) % 10


def half_ulp_interval(ref64: torch.Tensor, b64: torch.Tensor, dtype):
    """[round(ref - b), round(ref + b)] in ``dtype`` (as float64): where an fp32 value within b of ref can be stored"""
    return expected(ref64 - b64, dtype).to(F64), expected(ref64 + b64, dtype).to(F64)


def tree_sum_bound(rows: int, v64: torch.Tensor) -> float:
    return (math.ceil(rows / 256) + 8) * U * float(v64.abs().sum())
