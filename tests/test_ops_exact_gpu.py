"""gemm.hip (gemm, linear_bwd, colsum) and the pool backward kernels against the integer-exact oracle
(tests/_exact_oracle.py; tests/test_ops_exact_cpu.py ties it to torch's float64 ops and checks every case's
preconditions).  Every assertion is torch.equal over all elements of all outputs: with small-integer inputs every
fp32 partial sum is exact in any order, so there is no tolerance.  Each case first asserts through the plan query
(ops/plans.py: the structs the launchers dispatch on) that its launch takes the form its id names.

Compute dtypes: bf16 and fp16 (16-bit activations, fp32 weights) and fp32 (fp32 everything)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _exact_oracle as orc  # noqa: E402
from _exact_oracle import COLSUM_CASES, GEMM_CASES, LINEAR_BWD_CASES  # noqa: E402

from csed_514_project_distributed_training_using_pytorch_amd.ops import _native, plans  # noqa: E402
from csed_514_project_distributed_training_using_pytorch_amd.ops.rng import philox_uniform_reference  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
DTYPES = [torch.bfloat16, torch.float16, torch.float32]
MF = _native.MFMA_CODE
_CACHE: dict = {}


def _dt(dtype) -> str:
    return str(dtype).replace("torch.", "")


@pytest.fixture(scope="module", autouse=True)
def _module():
    _native.require()
    yield
    _CACHE.clear()


def _cached(key, make):
    """Inputs and references are computed once per case and shared by the dtype parametrisation."""
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def _exact(got: torch.Tensor, want64: torch.Tensor, what: str, dims: str) -> None:
    """got == the exact value through torch's conversion to got's dtype, everywhere."""
    got = got.detach().cpu()
    want = orc.expected(want64, got.dtype) if got.dtype != torch.uint8 else want64.to(torch.uint8)
    assert got.shape == want.shape, f"{what}: shape {tuple(got.shape)} != {tuple(want.shape)}"
    if torch.equal(got, want):
        return
    bad = torch.nonzero(~(got == want))  # (NaN counts as a mismatch)
    first = "; ".join(f"({dims}) = {tuple(i.tolist())}: expected {want[tuple(i)].item()} got {got[tuple(i)].item()}"
                      for i in bad[:5])
    raise AssertionError(f"{what}: {bad.shape[0]} of {got.numel()} elements differ; first {first}")


def _plan_is(plan, want: dict, what: str) -> None:
    for k, v in want.items():
        have = getattr(plan, k)
        if isinstance(v, dict):
            assert have is not None, f"{what}: plan has no {k}: {plan}"
            _plan_is(have, v, what + "." + k)
        else:
            assert have == v, f"{what}: plan.{k} = {have}, the case needs {v}: {plan}"


def test_maxpool_relu_backward_exact():
    """maxpool_relu_bwd's un-pooling rule (both of its kernels: even 2 x 2 planes, and the general one)."""
    o = _native.ops()
    g = torch.Generator().manual_seed(5)
    for shape in ((3, 5, 8, 12), (2, 3, 7, 9)):
        N, C, H, W = shape
        conv = orc.acts(g, shape)[:, :, :H // 2 * 2, :W // 2 * 2]
        scale = orc.scales(g, N * C)
        out, idx = orc.pool_ref(conv, scale)
        dyp = orc.grads(g, out.shape)
        want = torch.zeros(shape, dtype=torch.float64)
        want[:, :, :H // 2 * 2, :W // 2 * 2] = orc.unpool_ref(dyp, idx, out, scale)
        for dt in DTYPES:
            dx = torch.full(shape, float("nan"), device=DEV, dtype=dt)
            o.maxpool_relu_bwd(dyp.to(DEV, dt), out.to(DEV, dt), idx.to(DEV), scale.to(DEV, torch.float32), dx, 2)
            _exact(dx, want, f"maxpool_relu_bwd {shape} {_dt(dt)}", "n, c, h, w")


# ------------------------------------------------------------------- gemm
def _lay(t64: torch.Tensor, kind: str, dtype) -> torch.Tensor:
    """A logical [R, K] matrix on the GPU in the layout `kind` (see GemmCase)."""
    R, K = t64.shape
    if kind == "u8":
        return t64.to(DEV, torch.uint8)
    t = t64.to(DEV, dtype)
    if kind == "k":
        return t.contiguous()
    if kind == "r":
        return t.t().contiguous().t()
    if kind == "odd":
        buf = torch.zeros(R, K + 1, device=DEV, dtype=dtype)
        buf[:, :K] = t
        return buf[:, :K]
    assert kind == "off"
    buf = torch.zeros(R * K + 8, device=DEV, dtype=dtype)
    buf[1:1 + R * K] = t.reshape(-1)
    return buf[1:1 + R * K].view(R, K)


def _gemm_operands(c, d, dt):
    A = _lay(d["A"], c.la, dt)
    B = _lay(d["B"].t().contiguous(), c.lb, dt).t()  # (lb "k": B(k, n) contiguous along k, a weight's .t() view)
    G = None
    if c.gate:
        G = _lay(d["G"], c.la, torch.float32 if c.gate == "f32" else dt)
    cdt = torch.float32 if (c.c32 or dt == torch.float32) else dt
    C = d["C0"].to(DEV, cdt)
    bias = d["bias"].to(DEV, torch.float32) if c.bias else None
    rs = torch.full((c.M,), float("nan"), device=DEV) if c.rowsum else None
    return A, B, C, G, bias, rs


@pytest.mark.parametrize("dt", DTYPES, ids=_dt)
@pytest.mark.parametrize("c", GEMM_CASES, ids=lambda c: c.id)
def test_gemm_exact(c, dt):
    o = _native.ops()
    d = _cached(("gemm", c.id), lambda: orc.gemm_inputs(c))
    A, B, C, G, bias, rs = _gemm_operands(c, d, dt)
    want = c.plan32 if (dt == torch.float32 and c.plan32 is not None) else c.plan
    plan = plans.gemm_plan(A, B, C, dt, G, rs)
    _plan_is(plan, want, f"{c.id}[{_dt(dt)}]")
    if c.id == "block-gate-f32-demoted":
        # A alone would be staged as vectors along K; the fp32 gate has the same mode here (both aligned), and a
        # gate whose mode differs demotes A: shown on the same operands with a misaligned gate
        assert plan.a_mode == plans.K_CONTIG
        Goff = _lay(d["G"], "off", torch.float32)
        # (same sizes and strides as A, another base alignment)
        assert plans.gemm_plan(A, B, C, dt, Goff, rs).a_mode == plans.SCALAR
        G = Goff
    keep = None
    seed, offset = 1234, 3
    if c.act == 2:
        u = philox_uniform_reference(seed, offset, np.arange(c.M * c.N)).reshape(c.M, c.N)
        keep = torch.from_numpy(u >= 0.5).double() * 2.0
    o.gemm(A, B, C, bias, c.alpha, c.beta, c.act, 0.5 if c.act == 2 else 0.0, seed, offset, None, G, c.gs, MF[dt], rs)
    r = _cached(("gemmref", c.id), lambda: orc.gemm_refs(c, d, keep))
    _exact(C, r["C"], f"{c.id}[{_dt(dt)}] C", "m, n")
    if c.rowsum:
        _exact(rs, r["rowsum"], f"{c.id}[{_dt(dt)}] rowsum", "m")


@pytest.mark.parametrize("dt", DTYPES, ids=_dt)
@pytest.mark.parametrize("c", LINEAR_BWD_CASES, ids=lambda c: c.id)
def test_linear_bwd_exact(c, dt):
    """linear_bwd (the pair kernel where both GEMMs are small) == its two single gemm launches == the oracle."""
    o = _native.ops()
    d = _cached(("lbwd", c.id), lambda: orc.linear_bwd_inputs(c))
    r = _cached(("lbwdref", c.id), lambda: orc.linear_bwd_refs(c, d))
    dy, x, w = d["dy"].to(DEV, dt), d["x"].to(DEV, dt), d["w"].to(DEV, torch.float32)
    G = d["G"].to(DEV, dt) if c.gate else None
    dx, dw, db = torch.empty_like(x), torch.full_like(w, float("nan")), torch.full((c.O,), float("nan"), device=DEV)
    plan = plans.linear_bwd_plan(dy, x, w, dt, G, dx, dw, db)
    assert plan.pairable == c.pairable and len(plan.gemms) == 2, f"{c.id}: {plan}"
    o.linear_bwd(dy, x, w, G, c.gs, dx, dw, db, MF[dt])
    _exact(dx, r["dx"], f"{c.id} dx", "m, i")
    _exact(dw, r["dw"], f"{c.id} dw", "o, i")
    _exact(db, r["db"], f"{c.id} db", "o")
    # the two single launches
    dx1, dw1, db1 = torch.empty_like(dx), torch.empty_like(dw), torch.empty_like(db)
    o.gemm(dy, w, dx1, None, 1.0, 0.0, 0, 0.0, 0, 0, None, G, c.gs, MF[dt], None)
    o.gemm(dy.t(), x, dw1, None, 1.0, 0.0, 0, 0.0, 0, 0, None, G.t() if c.gate else None, c.gs, MF[dt], db1)
    assert torch.equal(dx1, dx) and torch.equal(dw1, dw) and torch.equal(db1, db), f"{c.id}: pair != single launches"


@pytest.mark.parametrize("dt", DTYPES, ids=_dt)
@pytest.mark.parametrize("c", COLSUM_CASES, ids=lambda c: c.id)
def test_colsum_exact(c, dt):
    d = orc.colsum_inputs(c)
    x = d["x"].to(DEV, dt)
    G = None if c.gate is None else d["G"].to(DEV, torch.float32 if c.gate == "f32" else dt)
    out = d["out0"].to(DEV, torch.float32)
    _native.ops().colsum(x, G, c.gs, out, c.beta)
    _exact(out, orc.colsum_refs(c, d)["out"], f"colsum {c.id}[{_dt(dt)}]", "col")
