"""The update oracle itself (tests/_update_oracle.py), without a GPU: its Python mirror of the layout
contract against the header compiled for the host, its gradient reference on a case computed by hand,
its SGD step against torch.optim.SGD in float64, and the condition the exact GPU tests rest on.  With
these green, a failure of tests/test_update_oracle_gpu.py points at the kernel, not at the oracle."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _update_oracle as orc  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


def _sections(text: str) -> dict:
    out, key = {}, None
    for line in text.splitlines():
        if line.startswith("# "):
            key = line[2:].strip()
            out[key] = []
        elif line.strip():
            out[key].append(int(line))
    return {k: np.array(v, dtype=np.int64) for k, v in out.items()}


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not available")
def test_layout_mirror_matches_the_header(tmp_path):
    exe = tmp_path / "update_oracle_layout"
    cmd = [HIPCC, "-O1", "-std=c++17", f"-I{os.path.join(ROOT, 'csrc')}",
           os.path.join(ROOT, "tests", "native", "update_oracle_layout.cpp"), "-o", str(exe)]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert b.returncode == 0, b.stderr[-3000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    sec = _sections(r.stdout)
    consts = [orc.NP, orc.O_C1W, orc.O_C1B, orc.O_C2W, orc.O_C2B, orc.O_F1W, orc.O_F1B, orc.O_F2W, orc.O_F2B, orc.CNP,
              orc.C1_CH, orc.S_C2, orc.CNP_PAD, orc.N_CHUNKS, orc.V_P2, orc.V_DZ1, orc.V_H, orc.V_DLOG, orc.VEC,
              orc.SPLIT_K]
    assert sec["constants"].tolist() == consts
    assert np.array_equal(sec["slab_slot"], orc.SLOT_OF_PARAM) and len(orc.SLOT_OF_PARAM) == orc.CNP
    assert np.array_equal(sec["slot_param"], orc.PARAM_OF_SLOT) and len(orc.PARAM_OF_SLOT) == orc.CNP_PAD
    for G, B in ((4, 1), (32, 8), (7, 100), (256, 64), (256, 1000)):
        R2 = min(G, B)
        mine = []
        for s in range(orc.CNP_PAD):
            rows = G if (s >> 6) < orc.C1_CH else R2
            mine += [int(orc.slab_off(s, min(row, rows - 1), G, R2)) for row in (0, 1, rows // 2, rows - 1)]
        assert np.array_equal(sec[f"slab_off {G} {B}"], np.array(mine)), (G, B)
        # the vectorised form fill() uses is the scalar one
        s = np.arange(orc.CNP_PAD, dtype=np.int64)
        assert np.array_equal(orc.slab_off(s, 0, G, R2), np.array(mine[0::4]))
        assert int(orc.slab_off(s, 0, G, R2).max()) < orc.slab_span(G, B) <= G * orc.CNP_PAD
    mine = [orc.vec16_index(f, b) for f in (0, 1, 319, 320, 383, 384, 448, 463) for b in (0, 1, 3, 4, 7, 63, 64, 1000, 2050)]
    assert sec["vec16_index"].tolist() == mine
    assert sec["vec16_bytes"].tolist() == [orc.round_up(B, 64) * orc.VEC * 2 for B in (1, 63, 64, 65, 1000, 2051)]


def test_reference_on_a_hand_computed_case():
    """grid 2, B 3: one non-zero row per chunk kind (conv1: workgroup 1; conv2 weight: sample row 0; conv2
    bias: sample row 1) and one non-zero sample (2).  The slots are written out by hand from the header's
    comment: conv2 weight (oc, k) at S_C2 + 20 k + oc, conv2 bias oc at S_C2 + 5000 + oc."""
    B, grid, gp = 3, 2, 0.25
    z = orc.make_inputs(B, grid, torch.float32, "int", 0)
    inp = orc.Inputs(torch.zeros_like(z.conv1), torch.zeros_like(z.conv2), torch.zeros_like(z.vec), z.loss)
    inp.conv1[1, 7] = 3.0  # conv1.weight[7]: slot 7
    inp.conv1[1, 255] = 1.0  # conv1.bias[5] = parameter 255: slot 255
    inp.conv2[0, 20 * 1 + 1] = -5.0  # conv2.weight (oc 1, k 1) = parameter 260 + 250 + 1
    inp.conv2[1, 5000 + 2] = 2.0  # conv2.bias[2] = parameter 5262
    inp.vec[2, orc.V_P2 + 5], inp.vec[2, orc.V_DZ1 + 3] = 2.0, -3.0
    inp.vec[2, orc.V_H + 7], inp.vec[2, orc.V_DLOG + 9] = 4.0, 1.5
    ref = orc.reference(inp, B, grid, gp)
    want = {7: 3.0, 255: 1.0, 511: -5.0, 5262: 2.0, 5280 + 3 * 320 + 5: -6.0, 21280 + 3: -3.0, 21330 + 9 * 50 + 7: 6.0,
            21830 + 9: 1.5}
    exp = torch.zeros(orc.NP, dtype=torch.float64)
    for k, v in want.items():
        exp[k] = v
    assert torch.equal(ref.sums, exp) and torch.equal(ref.grad, exp * gp) and torch.equal(ref.sabs, exp.abs())
    assert ref.n[:260].eq(grid).all() and ref.n[260:5280].eq(min(grid, B)).all() and ref.n[5280:].eq(B).all()
    assert ref.grad_post == gp


def test_make_inputs_respects_the_layout_contract():
    for dtype in (torch.bfloat16, torch.float16, torch.float32):
        for kind in ("int", "real"):
            inp = orc.make_inputs(70, 7, dtype, kind, 3)
            assert inp.conv1.shape == (7, 320) and inp.conv2.shape == (7, orc.CNP_PAD - 320)
            assert inp.vec.shape == (70, 464) and inp.loss.shape == (7, 2)
            for lo, hi in ((370, 384), (434, 448), (458, 464)):  # dZ1 50..63, H 50..63, dlogits 10..15
                assert not inp.vec[:, lo:hi].any()
            assert inp.vec[:, :320].any() and inp.vec[:, 320:370].any() and inp.vec[:, 448:458].any()
            assert not inp.conv1[:, 260:].any() and not inp.conv2[:, 5020:].any()
            if dtype != torch.float32:
                assert torch.equal(inp.vec.to(dtype).float(), inp.vec)  # representable in the compute dtype
            if kind == "int":
                assert inp.conv1.abs().max() <= 8 and inp.vec.abs().max() <= 4 and inp.loss.min() >= 0
                assert torch.equal(inp.vec, inp.vec.round())
    real32 = orc.make_inputs(70, 7, torch.float32, "real", 3).vec
    assert not torch.equal(real32.bfloat16().float(), real32)  # the fp32 layout's vectors are NOT 16-bit values


@pytest.mark.parametrize("mom,damp,wd,nesterov", orc.SGD_TABLE)
def test_sgd_reference_is_torch_sgd_in_float64(mom, damp, wd, nesterov):
    torch.manual_seed(2)
    n = 257
    p0 = torch.randn(n, dtype=torch.float64)
    ref = p0.clone().requires_grad_(True)
    opt = torch.optim.SGD([ref], lr=orc.f32(orc.LR), momentum=orc.f32(mom), dampening=orc.f32(damp),
                          weight_decay=orc.f32(wd), nesterov=nesterov)
    p, m = p0.clone(), torch.zeros(n, dtype=torch.float64)
    for step in range(3):
        g = torch.randn(n, dtype=torch.float64)
        ref.grad = g.clone()
        opt.step()
        # the lenet_update / lenet_sgd_kernel rule and the sgd_flat rule for ``first`` agree from a zero buffer
        pa, ma = orc.sgd_reference(p, m, g, step == 0 and damp != 0, orc.LR, mom, damp, wd, nesterov)
        pb, mb = orc.sgd_reference(p, m, g, step == 0, orc.LR, mom, damp, wd, nesterov)
        torch.testing.assert_close(pa, pb, rtol=1e-14, atol=1e-15)
        torch.testing.assert_close(ma, mb, rtol=1e-14, atol=1e-15)
        p, m = pa, ma
        torch.testing.assert_close(p, ref.detach(), rtol=1e-13, atol=1e-14)
        if mom != 0:
            torch.testing.assert_close(m, opt.state[ref]["momentum_buffer"], rtol=1e-13, atol=1e-14)
        else:
            assert not m.any()  # no buffer: untouched
    if damp != 0:  # a non-zero buffer at a first step is ignored: buf = g'
        _, m1 = orc.sgd_reference(p0, torch.ones(n), g, True, orc.LR, mom, damp, wd, nesterov)
        torch.testing.assert_close(m1, g + orc.f32(wd) * p0, rtol=1e-14, atol=1e-15)


def test_integer_sums_are_exact_in_fp32():
    """The exact GPU tests compare fp32 results bit for bit with the fp64 sums: every partial sum of the
    integer inputs must be an integer below 2^24, in any order -- so the sum of |addends| must be, at
    the largest batch and grid used (2051 on 256) and times the largest loopback world (8)."""
    B, grid = 2051, 256
    inp = orc.make_inputs(B, grid, torch.bfloat16, "int", 1)
    ref = orc.reference(inp, B, grid, 1.0)
    assert 8 * ref.sabs.max().item() < 2 ** 24
    assert 8 * max(grid * 8, B * 4 * 4) < 2 ** 24  # (the same from the value ranges alone)
    assert torch.equal(ref.sums, ref.sums.round()) and torch.equal(ref.sums.float().double(), ref.sums)
    assert inp.loss.sum(0).max().item() + 64 < 2 ** 24
