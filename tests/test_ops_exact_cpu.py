"""tests/_exact_oracle.py against torch's own float64 CPU ops on the oracle's integer inputs (exactly), the
preconditions of every case the GPU file runs, and the impulse family's index map.  No GPU."""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _exact_oracle as orc  # noqa: E402
from _exact_oracle import ALL_CASES, ColsumCase, GemmCase  # noqa: E402


def test_pool_references_equal_torch_float64():
    g = torch.Generator().manual_seed(3)
    c = orc.acts(g, (3, 5, 8, 12)).requires_grad_(True)
    scale = orc.scales(g, 15)
    out, idx = orc.pool_ref(c.detach(), scale)
    m, flat = F.max_pool2d(c.detach(), 2, return_indices=True)
    assert torch.equal(out, F.relu(m) * scale.view(3, 5, 1, 1))
    # torch's flat index of the maximum -> position inside the window (its tie rule: the first maximum)
    assert torch.equal(idx.long(), (flat // 12 % 2) * 2 + flat % 12 % 2)
    # the un-pooling rule is the pool's own backward (the ReLU and the scale on top of it)
    dyp = orc.grads(g, out.shape)
    (dc,) = torch.autograd.grad(F.relu(F.max_pool2d(c, 2)) * scale.view(3, 5, 1, 1), c, dyp)
    assert torch.equal(orc.unpool_ref(dyp, idx, out, scale), dc)


def test_pool_tie_rule_is_first_maximum():
    c = torch.tensor([[3.0, 3.0], [3.0, 3.0]]).view(1, 1, 2, 2).double()
    assert orc.pool_ref(c)[1].item() == 0
    c = torch.tensor([[1.0, 3.0], [3.0, 2.0]]).view(1, 1, 2, 2).double()
    assert orc.pool_ref(c)[1].item() == 1
    c = torch.tensor([[-5.0, -7.0], [-5.0, -4.0]]).view(1, 1, 2, 2).double()
    out, idx = orc.pool_ref(c)
    assert idx.item() == 3 and out.item() == 0.0
    # the un-pooling gates on the pooled output, not on the gradient
    assert orc.unpool_ref(torch.ones(1, 1, 1, 1), idx, out).abs().sum().item() == 0.0


@pytest.mark.parametrize("c", [GemmCase("plain", 17, 33, 45), GemmCase("ab", 33, 17, 64, alpha=0.5, beta=-2.0),
                               GemmCase("gate-rowsum", 50, 16, 64, gate="same", gs=2.0, rowsum=True, bias=False, act=1)],
                         ids=lambda c: c.id)
def test_gemm_references_equal_torch_float64(c):
    d = orc.gemm_inputs(c)
    r = orc.gemm_refs(c, d)
    A = d["A"] if not c.gate else d["A"] * (d["G"] > 0) * c.gs
    want = c.alpha * (A @ d["B"]) + c.beta * d["C0"] + (d["bias"] if c.bias else 0.0)
    assert torch.equal(r["C"], F.relu(want) if c.act else want)
    if c.rowsum:
        assert torch.equal(r["rowsum"], c.alpha * A.sum(1))


def test_colsum_reference():
    c = ColsumCase("g", 9, 33, beta=-2.0, gate="same", gs=2.0)
    d = orc.colsum_inputs(c)
    want = (d["x"] * (d["G"] > 0) * 2.0).sum(0) - 2.0 * d["out0"]
    assert torch.equal(orc.colsum_refs(c, d)["out"], want)


@pytest.mark.parametrize("c", ALL_CASES, ids=lambda c: type(c).__name__[:-4] + "-" + c.id)
def test_preconditions_of_every_gpu_case(c):
    orc.assert_exact_preconditions(c)


def test_linear_bwd_references_equal_torch_float64():
    c = orc.LINEAR_BWD_CASES[0]
    d = orc.linear_bwd_inputs(c)
    r = orc.linear_bwd_refs(c, d)
    x, w = d["x"].clone().requires_grad_(True), d["w"].clone().requires_grad_(True)
    y = F.linear(x, w, torch.zeros(c.O, dtype=torch.float64, requires_grad=True))
    gdy = d["dy"] * (d["G"] > 0) * c.gs
    dx, dw = torch.autograd.grad(y, (x, w), gdy)
    assert torch.equal(r["dx"], dx) and torch.equal(r["dw"], dw) and torch.equal(r["db"], gdy.sum(0))


def test_case_tables_hold_rounded_and_unrounded_outputs():
    """Per op, at least one case whose outputs pass 2048 (so bf16 and fp16 stores round; colsum's output is fp32,
    its big case only passes the mark) and one that stays within 256."""
    tables = (("gemm", [c for c in orc.GEMM_CASES if not c.impulse and c.act != 2 and c.M <= 600], orc.gemm_refs,
               orc.gemm_inputs, "C"),
              ("linear_bwd", orc.LINEAR_BWD_CASES, orc.linear_bwd_refs, orc.linear_bwd_inputs, "dx"),
              ("colsum", orc.COLSUM_CASES, orc.colsum_refs, orc.colsum_inputs, "out"))
    for op, cases, refs, inputs, key in tables:
        tops = {c.id: float(refs(c, inputs(c))[key].abs().max()) for c in cases}
        assert any(t > 2048 for t in tops.values()) and any(t <= 256 for t in tops.values()), (op, tops)


def test_preconditions_reject_overflow_and_fractions():
    with pytest.raises(AssertionError, match="2\\^24"):
        orc.assert_exact_preconditions(GemmCase("overflow", 1, 2, 1 << 22, big=True))
    with pytest.raises(AssertionError, match="neither"):
        orc.assert_exact_preconditions(GemmCase("alpha", 4, 4, 8, alpha=0.3))


def test_impulse_inputs_read_back_the_index_map():
    # GEMM: row m of C names B's row: C[m, n] = B[k(m), n] (+ 3 * B[k(m) + 256, n] past 256)
    c = GemmCase("imp", 33, 16, 1000, impulse=True, bias=False)
    d = orc.gemm_inputs(c)
    C = orc.gemm_refs(c, d)["C"]
    m = torch.arange(c.M)
    k = (m * 37) % c.K
    assert torch.equal(C, d["B"][k] + 3.0 * d["B"][(k + 256) % c.K])
