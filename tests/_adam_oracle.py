"""fp64 oracle of the Adam / AdamW rule that csed::lenet_update_adam applies (tests/test_adam_cpu.py ties
it to torch.optim.Adam / AdamW, tests/test_adam_gpu.py compares the kernels with it), and a derived bound
on what an fp32 evaluation of that rule may differ from it by.  Plain torch on the CPU, next to
tests/_update_oracle.py, whose ``f32`` it shares."""
from __future__ import annotations

import math

import torch

from _update_oracle import f32

U = 2.0 ** -24  # an fp32 rounding's relative error
# relative error allowed to the kernels' 1 - beta^t: log(beta) rounded to fp32 (1), t log(beta) rounded (1),
# expm1f at OpenCL's full-profile accuracy of 3 ulp = 6 u, which ROCm's device library meets -- 8 u.  The
# argument's two roundings are not amplified: |x e^x / (e^x - 1)| <= 1 for x < 0.
BC_ROUNDINGS = 8


def adam_reference(p, m, v, g, t: int, lr: float, betas, eps: float, wd: float, decoupled: bool):
    """One fp64 step number t (1-based) of torch.optim.Adam's (``decoupled``: AdamW's) rule, amsgrad=False,
    maximize=False, from parameters p, exp_avg m, exp_avg_sq v and gradient g:

        g' = g + wd p                      (Adam)      p = p (1 - lr wd), g' = g      (AdamW)
        m  = m + (1 - b1) (g' - m);        v = b2 v + (1 - b2) g'^2
        p -= lr / (1 - b1^t) * m / (sqrt(v) / sqrt(1 - b2^t) + eps)

    The hyper-parameters are first rounded to float32, as the kernels receive them.  Returns (p, m, v)."""
    lr, b1, b2, eps, wd = f32(lr), f32(betas[0]), f32(betas[1]), f32(eps), f32(wd)
    p, m, v, g = p.double(), m.double(), v.double(), g.double()
    if decoupled:
        p = p * (1.0 - lr * wd)
    else:
        g = g + wd * p
    m = m + (1.0 - b1) * (g - m)
    v = b2 * v + (1.0 - b2) * g * g
    bc1, bc2 = 1.0 - b1 ** t, 1.0 - b2 ** t
    p = p - (lr / bc1) * (m / (v.sqrt() / math.sqrt(bc2) + eps))
    return p, m, v


def adam_bounds(p, m, v, g, t: int, lr: float, betas, eps: float, wd: float, decoupled: bool):
    """Per-element bounds (m, v, p) on |fp32 evaluation - adam_reference| for one step from the same fp32
    state (p, m, v) and a gradient g that is exact in fp32.

    u = 2^-24.  Every fp32 operation below is correctly rounded (the build passes no fast-math flag, and
    hipcc's default keeps fp32 divide and sqrt correctly rounded), so it returns its exact result times
    (1 + d), |d| <= u; a fused multiply-add only removes roundings.  Each line counts roundings of terms
    that are at most the stated magnitude; (1 + u)^k - 1 <= (k + 1) u for the small k here.

    g' (Adam): wd p, g + wd p: 2 roundings of terms <= G = |g| + wd |p|:       |dg'| <= 3 u G  =: Eg
       (AdamW: g' = g exactly, G = |g|, Eg = 0.)
    m: m' = fma(c, d, m) with c = 1 - b1 and d = g' - m each rounded once: c's and d's roundings enter as
       u (1 - b1) |g' - m|, the fma's own as u |m'|, all three at most u M with M = (1 - b1) (G + |m|) + |m|;
       with one to spare and the inherited (1 - b1) Eg:          Em = 4 u M + (1 - b1) Eg
    v: v' = fma(c, s, w) with c = 1 - b2, s = g'^2 and w = b2 v each rounded once and the fma's own rounding:
       four roundings of terms <= V = (1 - b2) G^2 + b2 |v|, one to spare, plus the inherited error of
       g'^2, (1 - b2) (2 G Eg + Eg^2):                          Ev = 5 u V + (1 - b2) (2 G Eg + Eg^2)
    bias corrections: 1 - b^t to BC_ROUNDINGS u relative (see there), so step = lr / bc1 carries
       BC_ROUNDINGS + 1 roundings with the divide, and r = sqrt(bc2) BC_ROUNDINGS / 2 + 1.
    denominator D = sqrt(v') / r + eps (v' the new v, D >= eps > 0): |sqrt(a) - sqrt(b)| = |a - b| /
       (sqrt(a) + sqrt(b)) is at most |a - b| / sqrt(b) and at most sqrt(|a - b|) (the second for v' near
       0, where the first is unbounded), so Es = min(Ev / sqrt(v'), sqrt(Ev)) and
       E_D = (Es + sqrt(v') (1 + BC_ROUNDINGS / 2 + 1 + 1 + 1) u) / r + u D
           (sqrt's own rounding, r's error, the divide's rounding, one for the cross terms; then the sum's).
    quotient q = m' / D:  |dq| <= Em / (D - E_D) + |q| E_D / (D - E_D) + u |q|, with D - E_D the smallest
       denominator the fp32 evaluation can see (a bound needs D > E_D; it is infinite otherwise, and
       the tests keep eps large enough for that never to happen).
    p (Adam): step q and the difference, one fma: 1 rounding of a term <= |p| + step |q|, with step's
       BC_ROUNDINGS + 1:   Ep = step |dq| (1 + 10 u) + (BC_ROUNDINGS + 1) u step |q| + u (|p| + step |q|)
    p (AdamW) first multiplies p by 1 - lr wd: lr wd, the difference, the product: 3 roundings of terms
       <= |p| (1 + lr wd):  Ep += 4 u |p| (1 + lr wd).

    Nothing here is fitted to a kernel's output: tests/test_adam_cpu.py checks that a plain float32 torch
    evaluation of the rule stays inside these bounds."""
    lr, b1, b2, eps, wd = f32(lr), f32(betas[0]), f32(betas[1]), f32(eps), f32(wd)
    pa, ma, va, ga = p.double().abs(), m.double().abs(), v.double().abs(), g.double().abs()
    if decoupled:
        G, Eg = ga, torch.zeros_like(ga)
    else:
        G = ga + wd * pa
        Eg = 3 * U * G
    Em = 4 * U * ((1.0 - b1) * (G + ma) + ma) + (1.0 - b1) * Eg
    Ev = 5 * U * ((1.0 - b2) * G * G + b2 * va) + (1.0 - b2) * (2 * G * Eg + Eg * Eg)
    p1, m1, v1 = adam_reference(p, m, v, g, t, lr, (b1, b2), eps, wd, decoupled)
    bc1, bc2 = 1.0 - b1 ** t, 1.0 - b2 ** t
    step, r = lr / bc1, math.sqrt(bc2)
    D = v1.sqrt() / r + eps
    Es = torch.minimum(Ev / v1.sqrt().clamp_min(1e-300), Ev.sqrt())
    ED = (Es + v1.sqrt() * (BC_ROUNDINGS / 2 + 4) * U) / r + U * D
    q = (m1 / D).abs()
    room = D - ED
    dq = torch.where(room > 0, (Em + q * ED) / room.clamp_min(1e-300) + U * q, torch.full_like(q, math.inf))
    Ep = step * dq * (1 + 10 * U) + (BC_ROUNDINGS + 1) * U * step * q + U * (pa + step * q)
    if decoupled:
        Ep = Ep + 4 * U * pa * (1.0 + lr * wd)
    return Em, Ev, Ep
