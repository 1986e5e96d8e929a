"""For tests/test_adam_flat_cpu.py: the hyper-parameter table, the inputs
and the comparison with tests/_adam_oracle.py (imported, never copied: nothing here sets a tolerance)."""
from __future__ import annotations

import functools
import itertools
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _adam_oracle as ado  # noqa: E402

LR, EPS = 1e-3, 1e-8
BETAS = [(0.9, 0.999), (0.0, 0.999), (0.5, 0.9)]
# (decoupled, weight decay, betas): {Adam, AdamW} x wd in {0, 0.01} x the three beta pairs
HYPER = list(itertools.product([False, True], [0.0, 0.01], BETAS))
STARTS = [0, 999]  # steps already taken: zero moments, or non-zero ones and bias corrections at large t


def hyper_id(h) -> str:
    return "%s-wd%g-b%g-%g" % ("adamw" if h[0] else "adam", h[1], h[2][0], h[2][1])


@functools.lru_cache(maxsize=None)
def make_state(n: int, start: int, seed: int):
    """fp32 CPU (p, m, v) for a run that has taken ``start`` steps: zero moments at 0, else m of either sign
    and v >= 0 over twelve decades (every third m and every fifteenth v exactly 0).  Computed once per
    argument list and shared: callers copy, never write."""
    gen = torch.Generator().manual_seed(seed)
    p = torch.randn(n, generator=gen) * 0.25
    if start == 0:
        return p, torch.zeros(n), torch.zeros(n)
    m = torch.randn(n, generator=gen) * 0.1
    v = torch.rand(n, generator=gen) * 10.0 ** torch.randint(-12, 1, (n,), generator=gen).float()
    m[::3] = 0.0
    v[::15] = 0.0
    return p, m, v


@functools.lru_cache(maxsize=None)
def make_grads(n: int, steps: int, seed: int):
    """``steps`` fp32 CPU gradients over eight decades, a tenth of the elements exactly 0 (shared like
    make_state's)."""
    gen = torch.Generator().manual_seed(seed + 1000)
    out = []
    for _ in range(steps):
        g = torch.randn(n, generator=gen) * 10.0 ** torch.randint(-6, 2, (n,), generator=gen).float()
        g[torch.randperm(n, generator=gen)[: max(1, n // 10)]] = 0.0
        out.append(g)
    return out


def settle(g: torch.Tensor, p: torch.Tensor, gscale: float = 1.0) -> torch.Tensor:
    """g (on p's device) with the sign flipped wherever gscale * g + wd p would cancel to less than 5 % of
    |gscale g| + wd |p| at the table's non-zero weight decay (0.01).  Adam's g' = g + wd p then keeps at most
    20 times the relative error of its terms.  Where it cancels further the oracle's bound on the parameter
    is unbounded, and rightly so (tests/_adam_oracle.py: the fp32 denominator may vanish once |g'| is below
    about sqrt(11 u) = 8e-4 of |g| + wd |p|), so such an element can check nothing.  Applied to every case of
    the table alike, so all of them see the same inputs.

    Few elements may be touched, or the coupled-decay path would go unchecked; asserted here: at most 2 % (and
    one element of a tiny tensor).  A flip needs opposite signs and |gscale g| / (wd |p|) inside (19/21, 21/19),
    a window of 0.087 decades; make_grads draws log10 |g| as a uniform integer out of eight plus log10 |randn|,
    whose density peaks at 2 ln(10) phi(1) = 1.12 per decade, so at most 0.087 * 1.12 / 8 = 1.2 % of the
    elements fall in the window and half of those have the opposite sign: 0.6 %.  2 % leaves that a factor of
    three."""
    g = g.to(p.device)
    a, b = g.double() * gscale, 0.01 * p.double()
    near = (a + b).abs() < 0.05 * (a.abs() + b.abs())
    flipped = int(near.sum().item())
    assert flipped <= max(1, g.numel() // 50), f"settle flips {flipped} of {g.numel()} gradient elements"
    return torch.where(near, -g, g)


def check_step(got, prev, g, t: int, hyper, lr: float = LR, gscale: float = 1.0, what: str = ""):
    """``got`` = (p, m, v) after step number t from ``prev`` = (p, m, v) on gradient g * gscale (exact for a
    power of two): every element within adam_bounds of adam_reference, every bound finite.  The oracle runs on
    prev's device in fp64.  Returns the three bounds."""
    decoupled, wd, betas = hyper
    ge = g.to(prev[0].device).double() * gscale
    want = ado.adam_reference(*prev, ge, t, lr, betas, EPS, wd, decoupled)
    bounds = ado.adam_bounds(*prev, ge, t, lr, betas, EPS, wd, decoupled)
    for name, x, y, b in zip("mvp", (got[1], got[2], got[0]), (want[1], want[2], want[0]), bounds):
        assert bool(torch.isfinite(b).all()), f"{what} t {t} {name}: the bound is not finite everywhere"
        err = (x.to(y.device).double() - y).abs()
        worst = (err / b.clamp_min(1e-300)).max().item()
        assert bool((err <= b).all()), f"{what} t {t} {name}: worst error / bound {worst:.3f}"
    return bounds
