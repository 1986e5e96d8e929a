"""Integer-exact oracle of the GEMM library (csrc/kernels/gemm.hip: gemm, linear_bwd, colsum) and of the 2 x 2
max-pool + ReLU pair of elementwise.hip.  Host only: float64 torch, no GPU, none of the project's ops.

The kernels multiply 16-bit (or fp32) operands exactly and accumulate in fp32.  With small-integer inputs every
product and every partial sum is an integer below 2^24, so the fp32 result is exact in ANY summation order --
split-K partials, per-block slabs and their reduces included -- and a kernel must equal the references below bit
for bit at any batch size.  ``assert_exact_preconditions`` computes (not argues) that bound for a case.

Input families:
  * "int": activations and gradients in [-4, 4] (gradients with a share of exact zeros), weights in [-3, 3],
    biases in [-8, 8], channel scales in {0, 2}, gates with zeros and negatives.  ``big`` cases draw
    non-negative activations and weights so that outputs pass 256 (bf16) and 2048 (fp16) and are ROUNDED by the
    store: the expected value is the exact one through torch's fp32 -> 16-bit conversion (round to nearest
    even, the kernels' ``(T)x`` casts).  The other cases stay below, so a rounding disagreement can be told from
    an arithmetic one.
  * "impulse": a single 1 in an otherwise zero operand against an operand of distinct integers 1..K per
    256-block (a second impulse tells the blocks apart past 256): every output element names the operand
    element it read.

The pool's tie rule is part of the oracle (integers tie constantly): the first maximum in (row, column) order of
the 2 x 2 window -- maxpool_relu_fwd_kernel's strict ``>`` and torch's.  The argmax is taken on the unscaled
input; the value is relu(max) * scale, which for the scales in use (>= 0) equals scale, pool, ReLU in that order.
"""
from __future__ import annotations

from typing import NamedTuple

import torch

TWO24 = float(2 ** 24)
F64 = torch.float64
DTYPES = (torch.bfloat16, torch.float16, torch.float32)


# ------------------------------------------------------------------ inputs
def ints(gen: torch.Generator, shape, lo: int, hi: int, zero_share: float = 0.0) -> torch.Tensor:
    """Integer-valued float64 tensor, uniform in [lo, hi]; zero_share of it forced to exact zero."""
    t = torch.randint(lo, hi + 1, tuple(shape), generator=gen).to(F64)
    if zero_share > 0:
        t = t * (torch.rand(tuple(shape), generator=gen) >= zero_share)
    return t


def acts(gen, shape, big=False):
    return ints(gen, shape, 1 if big else -4, 4)


def grads(gen, shape):
    return ints(gen, shape, -4, 4, zero_share=0.25)


def weights(gen, shape, big=False):
    return ints(gen, shape, 1 if big else -3, 3)


def biases(gen, n):
    return ints(gen, (n,), -8, 8)


def scales(gen, n):
    return ints(gen, (n,), 0, 1) * 2.0


def gates(gen, shape):
    """The forward output a backward gates on: zeros, negatives and positives in about equal shares."""
    return ints(gen, shape, -2, 2)


def distinct(K: int) -> torch.Tensor:
    """1..256 repeating: distinct within each 256-block (exact in bf16, fp16 and fp32)."""
    return (torch.arange(K) % 256 + 1).to(F64)


def expected(exact: torch.Tensor, dtype: torch.dtype) -> torch.Tensor:
    """What a kernel must store for the exact value: fp32 as is, 16-bit through torch's RNE conversion."""
    return exact.to(torch.float32).to(dtype)


def round_trips(t: torch.Tensor, dtype: torch.dtype) -> bool:
    return bool(torch.equal(t.to(dtype).to(F64), t.to(F64)))


# -------------------------------------------------------------- references
def pool_ref(c, scale=None):
    """(relu(max of each 2 x 2 window) * scale[n, o], argmax byte = row * 2 + col of the FIRST maximum)"""
    c = c.to(F64)
    N, C, H, W = c.shape
    win = c.view(N, C, H // 2, 2, W // 2, 2).permute(0, 1, 2, 4, 3, 5).reshape(N, C, H // 2, W // 2, 4)
    best, idx = win[..., 0].clone(), torch.zeros(win.shape[:-1], dtype=torch.uint8)
    for r in range(1, 4):
        more = win[..., r] > best  # (strict: a tie keeps the earlier position)
        best = torch.where(more, win[..., r], best)
        idx = torch.where(more, torch.full_like(idx, r), idx)
    out = best.clamp_min(0)
    if scale is not None:
        out = out * scale.to(F64).view(N, C, 1, 1)
    return out, idx


def unpool_ref(dyp, idx, out, scale=None):
    """maxpool_relu_bwd's rule: the window position idx names gets dyp * scale where the pooled output is > 0"""
    dyp = dyp.to(F64)
    N, C, PH, PW = dyp.shape
    g = dyp * (out.to(F64) > 0)
    if scale is not None:
        g = g * scale.to(F64).view(N, C, 1, 1)
    win = torch.zeros(N, C, PH, PW, 4, dtype=F64)
    win.scatter_(4, idx.long().unsqueeze(-1), g.unsqueeze(-1))
    return win.view(N, C, PH, PW, 2, 2).permute(0, 1, 2, 4, 3, 5).reshape(N, C, PH * 2, PW * 2)


def gate_ref(dy, gate, gs):
    """linear_bwd's gated dY: dy * gs where the forward output is > 0, else 0"""
    return torch.where(gate.to(F64) > 0, dy.to(F64) * gs, torch.zeros((), dtype=F64))


def gemm_ref(A, B, C0=None, bias=None, alpha=1.0, beta=0.0, act=0, keep_scale=None):
    """act(alpha * A @ B + beta * C0 + bias): act 0 none, 1 ReLU, 2 ReLU x keep_scale[m, n]"""
    v = alpha * torch.einsum("mk,kn->mn", A.to(F64), B.to(F64))
    if beta != 0:
        v = v + beta * C0.to(F64)
    if bias is not None:
        v = v + bias.to(F64).view(1, -1)
    if act >= 1:
        v = v.clamp_min(0)
    if act == 2:
        v = v * keep_scale.to(F64)
    return v


def rowsum_ref(A, alpha=1.0):
    """The ones column: alpha * sum_k A[m, k]"""
    return alpha * A.to(F64).sum(1)


def colsum_ref(x, out0, beta=0.0, gate=None, gs=1.0):
    x = x.to(F64) if gate is None else gate_ref(x, gate, gs)
    return x.sum(0) + (beta * out0.to(F64) if beta != 0 else 0.0)


# ------------------------------------------------------------------- cases
class GemmCase(NamedTuple):
    """alpha * A @ B + beta * C + bias with act; la / lb: operand layouts ("k": K-contiguous, "r": row-contiguous
    (.t() of a [K, rows] buffer), "odd": K-contiguous with a row stride that is no multiple of 16 bytes, "off":
    base pointer one element past alignment, "u8": a uint8 operand); c32: fp32 C under 16-bit compute; gate: A is
    gated (None | "same" dtype | "f32"); rowsum: the ones column; plan: expected plan fields (plan32: under fp32
    compute, where they differ -- none of the cases below: a row of 4-byte elements is whole 16-byte vectors
    wherever the same row of 2-byte elements is, and no case has a stride that is a multiple of 4 but not 8)."""
    id: str
    M: int
    N: int
    K: int
    la: str = "k"
    lb: str = "k"
    alpha: float = 1.0
    beta: float = 0.0
    bias: bool = True
    act: int = 0
    c32: bool = True
    gate: str | None = None
    gs: float = 1.0
    rowsum: bool = False
    big: bool = False
    impulse: bool = False
    plan: dict = {}
    seed: int = 0
    plan32: dict | None = None


def gemm_inputs(c: GemmCase) -> dict:
    g = torch.Generator().manual_seed(2000 + c.seed)
    if c.impulse:
        A = torch.zeros(c.M, c.K, dtype=F64)
        m = torch.arange(c.M)
        A[m, (m * 37) % c.K] = 1.0
        if c.K > 256:
            A[m, ((m * 37) % c.K + 256) % c.K] += 3.0  # (tells the 256-blocks of B's values apart)
        B = ((torch.arange(c.K).view(c.K, 1) + torch.arange(c.N).view(1, c.N)) % 256 + 1).to(F64)
    else:
        A = ints(g, (c.M, c.K), 0, 4) if c.la == "u8" else (grads(g, (c.M, c.K)) if c.gate else acts(g, (c.M, c.K), c.big))
        B = ints(g, (c.K, c.N), 0, 3) if c.lb == "u8" else weights(g, (c.K, c.N), c.big)
    d = dict(A=A, B=B, C0=ints(g, (c.M, c.N), -4, 4))
    if c.bias:
        d["bias"] = biases(g, c.N)
    if c.gate:
        d["G"] = gates(g, (c.M, c.K))
    return d


def gemm_refs(c: GemmCase, d: dict, keep_scale=None, magnitude=False) -> dict:
    a = (lambda t: t.abs()) if magnitude else (lambda t: t)
    A = a(d["A"]) if not c.gate else (a(d["A"]) * abs(c.gs) if magnitude else gate_ref(d["A"], d["G"], c.gs))
    bias = a(d["bias"]) if c.bias else None
    if magnitude:
        r = dict(C=gemm_ref(A, a(d["B"]), a(d["C0"]), bias, abs(c.alpha), abs(c.beta), 0))
    else:
        r = dict(C=gemm_ref(A, d["B"], d["C0"], bias, c.alpha, c.beta, c.act, keep_scale))
    if c.rowsum:
        r["rowsum"] = rowsum_ref(A, abs(c.alpha) if magnitude else c.alpha)
    return r


class ColsumCase(NamedTuple):
    id: str
    rows: int
    cols: int
    beta: float = 0.0
    gate: str | None = None
    gs: float = 1.0
    big: bool = False


def colsum_inputs(c: ColsumCase) -> dict:
    g = torch.Generator().manual_seed(3000 + c.rows * 64 + c.cols)
    d = dict(x=acts(g, (c.rows, c.cols), True) if c.big else grads(g, (c.rows, c.cols)), out0=ints(g, (c.cols,), -9, 9))
    if c.gate:
        d["G"] = gates(g, (c.rows, c.cols))
    return d


def colsum_refs(c: ColsumCase, d: dict, magnitude=False) -> dict:
    if magnitude:
        return dict(out=colsum_ref(d["x"].abs() * abs(c.gs), d["out0"].abs(), abs(c.beta)))
    return dict(out=colsum_ref(d["x"], d["out0"], c.beta, d.get("G"), c.gs))


class LinearBwdCase(NamedTuple):
    """nn.Linear's backward on dy [M, O], x [M, I], w [O, I]: dx = gate(dy) w, dw = gate(dy)^T x, db = its row sums;
    pairable: both GEMMs in one launch of the pair kernel (the plan query's answer the case is named for)."""
    id: str
    M: int
    O: int
    I: int
    gate: bool = False
    gs: float = 1.0
    pairable: int = 1
    big: bool = False


def linear_bwd_inputs(c: LinearBwdCase) -> dict:
    g = torch.Generator().manual_seed(4000 + c.M + c.O)
    d = dict(dy=acts(g, (c.M, c.O), True) if c.big else grads(g, (c.M, c.O)), x=acts(g, (c.M, c.I), c.big),
             w=weights(g, (c.O, c.I), c.big))
    if c.gate:
        d["G"] = gates(g, (c.M, c.O))
    return d


def linear_bwd_refs(c: LinearBwdCase, d: dict, magnitude=False) -> dict:
    a = (lambda t: t.abs()) if magnitude else (lambda t: t)
    gdy = a(d["dy"])
    if c.gate:
        gdy = gdy * abs(c.gs) if magnitude else gate_ref(d["dy"], d["G"], c.gs)
    return dict(dx=gemm_ref(gdy, a(d["w"])), dw=gemm_ref(gdy.t(), a(d["x"])), db=rowsum_ref(gdy.t()))


def _is_small(v: float) -> bool:
    """alpha / beta / gate scale: a power of two or a small integer"""
    v = abs(float(v))
    return v == 0 or (v == int(v) and v <= 16) or (v > 0 and (2.0 ** round(torch.log2(torch.tensor(v)).item())) == v)


def assert_exact_preconditions(case) -> None:
    """Every input round-trips through each dtype it is given in, and for every output element the sum of
    |a||b| over its terms (bias, beta and alpha terms included) is below 2^24: then every partial sum in any
    order is an integer (or, alpha = 1/2, a half-integer far below 2^23) that fp32 holds exactly."""
    if isinstance(case, GemmCase):
        d = gemm_inputs(case)
        mags = gemm_refs(case, d, magnitude=True)
        scalars = (case.alpha, case.beta, case.gs)
    elif isinstance(case, LinearBwdCase):
        d = linear_bwd_inputs(case)
        mags = linear_bwd_refs(case, d, magnitude=True)
        scalars = (case.gs,)
    else:
        d = colsum_inputs(case)
        mags = colsum_refs(case, d, magnitude=True)
        scalars = (case.beta, case.gs)
    for name, t in d.items():
        assert torch.equal(t, t.round()), f"{case.id}: {name} is not integer-valued"
        u8 = isinstance(case, GemmCase) and ((name == "A" and case.la == "u8") or (name == "B" and case.lb == "u8"))
        for dt in ((torch.uint8,) if u8 else DTYPES):
            assert round_trips(t, dt), f"{case.id}: {name} does not round-trip through {dt}"
    for s in scalars:
        assert _is_small(s), f"{case.id}: scalar {s} is neither a power of two nor a small integer"
    for name, m in mags.items():
        top = float(m.abs().max())
        assert top < TWO24, f"{case.id}: {name}: sum of |a||b| reaches {top:.0f} >= 2^24"


# The case tables of tests/test_ops_exact_gpu.py (here, so that tests/test_ops_exact_cpu.py checks every case's
# preconditions without a GPU).  Shapes follow the launch conditions of launch_gemm; each case's plan fields are
# asserted through the plan query before the kernel runs.
GEMM_CASES = (
    [GemmCase(f"small-M{m}-N{n}-K{k}", m, n, k, plan=dict(small=1, splits=1), seed=i)
     for i, (m, n, k) in enumerate([(1, 1, 1), (15, 17, 16), (16, 16, 33), (17, 33, 15), (33, 15, 17), (16, 1, 16),
                                    (33, 33, 33)])] +
    [
        GemmCase("small-K1000", 33, 17, 1000, plan=dict(small=1)),
        GemmCase("small-K1024-big", 17, 33, 1024, big=True, plan=dict(small=1, a_mode=1, b_mode=1)),
        GemmCase("small-K1024-impulse", 33, 16, 1024, impulse=True, bias=False, plan=dict(small=1, a_mode=1, b_mode=1)),
        GemmCase("small-scalar-impulse", 33, 16, 1000, la="r", lb="r", impulse=True, bias=False,
                 plan=dict(small=1, a_mode=0, b_mode=0)),
        GemmCase("small-rowsum-N16", 50, 16, 64, la="r", rowsum=True, bias=False, plan=dict(small=1, tiles=8)),
        GemmCase("small-gate-same", 64, 50, 320, gate="same", gs=2.0, bias=False, plan=dict(small=1, a_mode=1)),
        GemmCase("small-gate-f32", 64, 50, 320, gate="f32", gs=1.0, bias=False, plan=dict(small=1)),
        GemmCase("small-u8-A", 33, 17, 100, la="u8", plan=dict(small=1, a_mode=0)),
        GemmCase("small-relu-16bitC", 37, 70, 45, act=1, c32=False, plan=dict(small=1)),
        GemmCase("small-relu-drop", 64, 50, 320, act=2, plan=dict(small=1)),
        # ---- gemm_kernel
        GemmCase("block-M4096-N320-K50", 4096, 320, 50, la="odd", plan=dict(small=0, splits=1, tiles=320, a_mode=0)),
        GemmCase("block-M4096-N320-K56-relu", 4096, 320, 56, act=1, c32=False, plan=dict(small=0, splits=1, a_mode=1, b_mode=1)),
        GemmCase("block-big-K1056", 70, 130, 1056, big=True, plan=dict(small=0)),
        GemmCase("split64-M50-N320-K4096", 50, 320, 4096, la="r", lb="r", plan=dict(small=0, splits=64, a_mode=0, b_mode=2)),
        GemmCase("block-rcontig-M72", 72, 64, 1056, la="r", lb="r", plan=dict(small=0, a_mode=2, b_mode=2)),
        GemmCase("split64-impulse", 50, 320, 4096, la="r", lb="r", impulse=True, bias=False, plan=dict(splits=64)),
        # (gemm_splits never returns 2: fewer than 256 tiles give cdiv(512, tiles) >= 3, and ktiles / 2 == 2 means
        # fewer than the 8 K-tiles a split needs.  3 is the smallest; K = 270 leaves the last of 4 splits empty)
        GemmCase("split3-K1100", 2240, 320, 1100, plan=dict(small=0, splits=3, tiles=175)),
        GemmCase("split4-K270-empty-last", 1100, 300, 270, la="odd", plan=dict(small=0, splits=4)),
        GemmCase("split-odd-K2085", 130, 200, 2085, la="off", lb="odd", plan=dict(small=0, a_mode=0, b_mode=0)),
        GemmCase("split-rowsum-N64", 50, 64, 4096, la="r", lb="r", rowsum=True, bias=False, plan=dict(small=0, grid_x=2)),
        GemmCase("block-gate-f32-demoted", 2100, 64, 1056, gate="f32", gs=2.0, bias=False, plan=dict(small=0)),
        GemmCase("block-gate-same", 2100, 64, 1056, gate="same", gs=1.0, bias=False, plan=dict(small=0, a_mode=1)),
        GemmCase("block-u8-B", 1100, 17, 1030, lb="u8", plan=dict(small=0, b_mode=0)),
        GemmCase("block-impulse-k", 1100, 40, 1056, impulse=True, bias=False, plan=dict(small=0, a_mode=1, b_mode=1)),
    ] +
    # ---- the epilogue's alpha / beta, onto fp32 and 16-bit C, on both kernels and through the split-K reduce
    [GemmCase(f"{name}-alpha{al}-beta{be}-{'c32' if c32 else 'c16'}", m, n, k, alpha=al, beta=be, c32=c32, plan=plan,
              seed=40 + j)
     for name, m, n, k, plan in [("small", 33, 17, 64, dict(small=1)), ("split", 50, 320, 2048, dict(small=0))]
     for j, (al, be, c32) in enumerate([(2.0, 1.0, True), (0.5, -2.0, True), (2.0, -2.0, False), (0.5, 1.0, False)])]
)

LINEAR_BWD_CASES = [
    LinearBwdCase("pair-M64-fc1", 64, 50, 320, True, 2.0, 1),
    LinearBwdCase("pair-M37-fc2", 37, 10, 50, False, 1.0, 1),
    LinearBwdCase("pair-M16-O512-big", 16, 512, 16, False, 1.0, 1, big=True),  # (dx passes 2048: a rounded 16-bit store)
    LinearBwdCase("single-M4096-fc1", 4096, 50, 320, True, 2.0, 0),
]

COLSUM_CASES = [ColsumCase(f"r{r}-c{c}", r, c, beta=be, gate=ga, gs=gs)
                for r, c, be, ga, gs in [(1, 1, 0.0, None, 1.0), (7, 31, 1.0, None, 1.0), (8, 32, 0.0, "same", 2.0),
                                         (9, 33, -2.0, "f32", 1.0), (1000, 33, 1.0, "same", 2.0), (1000, 1, 0.0, None, 1.0)]]
COLSUM_CASES.append(ColsumCase("r1000-c33-big", 1000, 33, big=True))  # (sums past 2048; the output is fp32 all the same)

ALL_CASES = list(GEMM_CASES) + LINEAR_BWD_CASES + COLSUM_CASES
