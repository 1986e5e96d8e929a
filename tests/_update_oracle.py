"""fp64 oracle of csed::lenet_update and the SGD kernels (tests/test_update_oracle_cpu.py ties it to
the header, tests/test_update_oracle_gpu.py compares the kernels with it).  Plain numpy / torch on the
CPU: a Python mirror of the layout contract in csrc/kernels/lenet_layout.h, synthetic slabs written
through that mirror, the gradient lenet_update must form from them as plain fp64 sums, and one fp64
step of torch's SGD rule.  No GPU code here: ``fill`` only copies into an engine's buffers."""
from __future__ import annotations

from typing import NamedTuple

import numpy as np
import torch

# ---------------------------------------------------------------- layout mirror (lenet_layout.h)
NP = 21840
O_C1W, O_C1B, O_C2W, O_C2B, O_F1W, O_F1B, O_F2W, O_F2B = 0, 250, 260, 5260, 5280, 21280, 21330, 21830
CNP = O_F1W
C1_CH = 5
S_C2 = C1_CH * 64
CNP_PAD = S_C2 + ((CNP - O_C2W) + 63) // 64 * 64
N_CHUNKS = CNP_PAD // 64
V_P2, V_DZ1, V_H, V_DLOG, VEC = 0, 320, 384, 448, 464
SPLIT_K = 4
# features the training kernels write (the others of each block stay zero)
N_P2, N_DZ1, N_H, N_DLOG = 320, 50, 50, 10


def slab_slot(p: int) -> int:
    """Slab slot of conv parameter p (conv2's slots are column-major in its wgrad GEMM)."""
    if p < O_C2W:
        return p
    if p < O_C2B:
        return S_C2 + ((p - O_C2W) % 250) * 20 + (p - O_C2W) // 250
    return S_C2 + 250 * 20 + (p - O_C2B)


def slot_param(s: int) -> int:
    """Parameter of slab slot s, -1 for padding."""
    if s < O_C2W:
        return s
    if s < S_C2:
        return -1
    t = s - S_C2
    if t >= 251 * 20:
        return -1
    return O_C2W + (t % 20) * 250 + t // 20 if t // 20 < 250 else O_C2B + t % 20


def slab_off(s, row, G, R2):
    """Float offset of (slot, row) in the slab: [chunk][row][64], G rows in a conv1 chunk and
    R2 = min(G, B) in a conv2 chunk.  Works on ints and on numpy arrays alike."""
    c = s >> 6
    r = np.where(c < C1_CH, c * G + row, C1_CH * (G - R2) + c * R2 + row)
    return r * 64 + (s & 63)


def slab_span(G: int, B: int) -> int:
    """Floats the (G, B) layout covers."""
    return (C1_CH * G + (N_CHUNKS - C1_CH) * min(G, B)) * 64


def vec16_index(f: int, b: int) -> int:
    """16-bit element index of feature f of sample b (sample quads, [B / 4][VEC][4])."""
    return ((b >> 2) * VEC + f) * 4 + (b & 3)


SLOT_OF_PARAM = np.array([slab_slot(p) for p in range(CNP)], dtype=np.int64)
PARAM_OF_SLOT = np.array([slot_param(s) for s in range(CNP_PAD)], dtype=np.int64)


def round_up(n: int, m: int) -> int:
    return (n + m - 1) // m * m


# ---------------------------------------------------------------- inputs
class Inputs(NamedTuple):
    conv1: torch.Tensor  # fp32 [grid, 320]: a row per workgroup, by slab slot 0..319 (padding slots zero)
    conv2: torch.Tensor  # fp32 [min(grid, B), CNP_PAD - 320]: a row per sample row, by slab slot - 320
    vec: torch.Tensor  # fp32 [B, 464]: P2 | dZ1 | H | dlogits per sample
    loss: torch.Tensor  # fp32 [grid, 2]: (loss, correct) partials per workgroup


def _written_features() -> torch.Tensor:
    m = torch.zeros(VEC, dtype=torch.bool)
    for off, n in ((V_P2, N_P2), (V_DZ1, N_DZ1), (V_H, N_H), (V_DLOG, N_DLOG)):
        m[off:off + n] = True
    return m


def make_inputs(B: int, grid: int, dtype: torch.dtype, kind: str, seed: int) -> Inputs:
    """Synthetic inputs of one lenet_update launch.  ``kind="int"``: small integers (slab [-8, 8],
    vectors [-4, 4], loss partials [0, 8]: exact in bf16 / fp16, every sum exact in fp32);
    ``kind="real"``: standard normal, the vectors rounded to the 16-bit compute dtype (full fp32 for
    the fp32 layout).  Feature rows the training kernels never write stay zero."""
    gen = torch.Generator().manual_seed(seed)
    R2 = min(grid, B)
    pad1 = torch.from_numpy(PARAM_OF_SLOT[:S_C2] < 0)
    pad2 = torch.from_numpy(PARAM_OF_SLOT[S_C2:] < 0)
    if kind == "int":
        conv1 = torch.randint(-8, 9, (grid, S_C2), generator=gen).float()
        conv2 = torch.randint(-8, 9, (R2, CNP_PAD - S_C2), generator=gen).float()
        vec = torch.randint(-4, 5, (B, VEC), generator=gen).float()
        loss = torch.randint(0, 9, (grid, 2), generator=gen).float()
    elif kind == "real":
        conv1 = torch.randn((grid, S_C2), generator=gen)
        conv2 = torch.randn((R2, CNP_PAD - S_C2), generator=gen)
        vec = torch.randn((B, VEC), generator=gen)
        if dtype != torch.float32:
            vec = vec.to(dtype).float()
        loss = torch.rand((grid, 2), generator=gen)
    else:
        raise ValueError(kind)
    conv1[:, pad1] = 0.0
    conv2[:, pad2] = 0.0
    vec[:, ~_written_features()] = 0.0
    return Inputs(conv1, conv2, vec, loss)


_NAN16 = {torch.bfloat16: 0x7FC0, torch.float16: 0x7E00}


def fill(eng, inputs: Inputs, B: int, grid: int, poison: bool = True) -> None:
    """Write ``inputs`` into the engine's slab (through slab_off), vector slab (through
    set_fc_vectors) and loss partials for a launch of per-rank batch B on ``grid`` workgroups.
    ``poison``: everything that launch must not use holds NaN -- slab floats outside the (grid, B)
    layout's span, slab padding slots, the vector slab's samples from B on, loss partials from
    ``grid`` on.  Without it those hold zeros."""
    R2 = min(grid, B)
    span = slab_span(grid, B)
    assert span <= eng.slab.numel(), f"(grid {grid}, B {B}) needs {span} slab floats, the engine has {eng.slab.numel()}"
    assert 2 * grid <= eng.loss_parts.numel() and round_up(B, 64) <= eng.vslab.shape[0]
    bad = float("nan") if poison else 0.0
    flat = torch.full((eng.slab.numel(),), bad, dtype=torch.float32)
    view = flat.numpy()
    pad = PARAM_OF_SLOT < 0
    for rows, s0, s1, vals in ((grid, 0, S_C2, inputs.conv1), (R2, S_C2, CNP_PAD, inputs.conv2)):
        s = np.arange(s0, s1, dtype=np.int64)[None, :]
        r = np.arange(rows, dtype=np.int64)[:, None]
        v = vals.numpy().copy()
        v[:, pad[s0:s1]] = bad
        view[slab_off(s, r, grid, R2)] = v
    eng.slab.view(-1).copy_(flat)
    rows = round_up(B, 64)
    v = torch.full((rows, VEC), bad, dtype=torch.float32)
    v[:B] = inputs.vec
    eng.set_fc_vectors(v)  # (zeroes the whole vector slab first)
    if poison:
        if eng.fp32:
            eng.vslab[B:].fill_(bad)
        else:
            eng.vslab.view(-1).view(torch.int16)[rows * VEC:].fill_(_NAN16[eng.compute_dtype])
    lp = torch.full((eng.loss_parts.numel(),), bad, dtype=torch.float32)
    lp[:2 * grid] = inputs.loss.reshape(-1)
    eng.loss_parts.copy_(lp)


# ---------------------------------------------------------------- references
class Reference(NamedTuple):
    grad: torch.Tensor  # fp64 [NP]: sums x float32(grad_post)
    sabs: torch.Tensor  # fp64 [NP]: sum of |addends| per element
    n: torch.Tensor  # int64 [NP]: addends per element
    sums: torch.Tensor  # fp64 [NP]: the sums before grad_post
    grad_post: float  # grad_post as the kernel receives it (rounded to float32)


def reference(inputs: Inputs, B: int, grid: int, grad_post: float) -> Reference:
    """What lenet_update must reduce ``inputs`` to, in flat parameter order, in fp64: a conv
    parameter is the sum of its slot over its chunk's rows; fc1.w = dZ1^T P2, fc1.b = sum dZ1,
    fc2.w = dlogits^T H, fc2.b = sum dlogits over the B samples; all times grad_post (the float32
    the kernel receives).  With it, per element, the sum of |addends| and their number."""
    R2 = min(grid, B)
    assert inputs.conv1.shape == (grid, S_C2) and inputs.conv2.shape == (R2, CNP_PAD - S_C2) and inputs.vec.shape == (B, VEC)
    c1, c2, v = inputs.conv1.double(), inputs.conv2.double(), inputs.vec.double()
    sums, sabs = torch.zeros(NP, dtype=torch.float64), torch.zeros(NP, dtype=torch.float64)
    n = torch.zeros(NP, dtype=torch.int64)
    slots = torch.from_numpy(SLOT_OF_PARAM)
    in1 = slots < S_C2
    p1, p2 = torch.nonzero(in1).flatten(), torch.nonzero(~in1).flatten()
    sums[p1], sabs[p1], n[p1] = c1[:, slots[p1]].sum(0), c1[:, slots[p1]].abs().sum(0), grid
    sums[p2], sabs[p2], n[p2] = c2[:, slots[p2] - S_C2].sum(0), c2[:, slots[p2] - S_C2].abs().sum(0), R2
    p2v, dz1 = v[:, V_P2:V_P2 + N_P2], v[:, V_DZ1:V_DZ1 + N_DZ1]
    h, dlog = v[:, V_H:V_H + N_H], v[:, V_DLOG:V_DLOG + N_DLOG]
    for off, a, b in ((O_F1W, dz1, p2v), (O_F2W, dlog, h)):
        sums[off:off + a.shape[1] * b.shape[1]] = (a.t() @ b).reshape(-1)
        sabs[off:off + a.shape[1] * b.shape[1]] = (a.abs().t() @ b.abs()).reshape(-1)
    for off, a in ((O_F1B, dz1), (O_F2B, dlog)):
        sums[off:off + a.shape[1]] = a.sum(0)
        sabs[off:off + a.shape[1]] = a.abs().sum(0)
    n[O_F1W:] = B
    gp = float(np.float32(grad_post))
    return Reference(sums * gp, sabs, n, sums, gp)


def f32(x: float) -> float:
    """x as the kernels receive it: rounded to float32."""
    return float(np.float32(x))


def sgd_reference(p: torch.Tensor, m: torch.Tensor, g: torch.Tensor, first: bool, lr: float, mom: float,
                  damp: float, wd: float, nesterov: bool) -> tuple[torch.Tensor, torch.Tensor]:
    """One fp64 step of torch.optim.SGD's rule from parameters p, momentum buffer m and gradient g:
    g' = g + wd p;  buf = g' if ``first`` else mom m + (1 - damp) g';  d = g' + mom buf (nesterov) or
    buf;  p -= lr d.  With mom == 0 there is no buffer: d = g' and m comes back unchanged.  The
    hyperparameters are first rounded to float32, as the kernels receive them.  ``first``: for
    lenet_update / lenet_sgd_kernel, step counter 0 and damp != 0 (with zero dampening their zero
    buffer gives the same); for sgd_flat, step counter 0.  Returns (p, buf) in fp64."""
    lr, mom, damp, wd = f32(lr), f32(mom), f32(damp), f32(wd)
    p, m, g = p.double(), m.double(), g.double()
    gj = g + wd * p
    if mom == 0.0:
        return p - lr * gj, m.clone()
    buf = gj.clone() if first else mom * m + (1.0 - damp) * gj
    d = gj + mom * buf if nesterov else buf
    return p - lr * d, buf


def sgd_bounds(p: torch.Tensor, m: torch.Tensor, g: torch.Tensor, lr: float, mom: float, wd: float
               ) -> tuple[torch.Tensor, torch.Tensor]:
    """Per-element bounds (buffer, parameter) on |fp32 kernel - sgd_reference| for one step.

    With u = 2^-24 (an fp32 rounding's relative error) and S = |g| + wd |p| + mom |m|, every
    intermediate of the rule is at most S in magnitude, and the kernels round at most: g scale (sgd_flat
    only), wd p, g + wd p, 1 - damp, (1 - damp) g', the buffer's fma -- 6 roundings of terms <= S, so
    |buf error| <= ((1 + u)^6 - 1) S < 8 u S.  d adds one fma (nesterov) on a value <= (1 + mom) S, the
    parameter one more fma on a value <= |p| + lr |d|:  |p error| <= u (|p| + lr (1 + mom) S) +
    lr 7 u (1 + mom) S <= 8 u (|p| + lr (1 + mom) S).  A fused multiply-add only removes roundings."""
    u = 2.0 ** -24
    lr, mom, wd = f32(lr), f32(mom), f32(wd)
    p, m, g = p.double().abs(), m.double().abs(), g.double().abs()
    s = g + wd * p + mom * m
    return 8 * u * s, 8 * u * (p + lr * (1.0 + mom) * s)


# (momentum, dampening, weight_decay, nesterov) of every SGD test; lr = LR
SGD_TABLE = [(0.0, 0.0, 0.0, False), (0.0, 0.0, 1e-3, False), (0.5, 0.0, 0.0, False), (0.9, 0.0, 5e-4, True),
             (0.9, 0.3, 1e-3, False), (0.5, 0.1, 0.0, False)]
LR = 0.05
