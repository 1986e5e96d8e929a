"""tests/_elementwise_oracle.py against torch's own float64 ops and hand-computed cases, and the preconditions of
every exact case of tests/test_elementwise_oracle_gpu.py.  No GPU."""
import os
import sys
from fractions import Fraction

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _elementwise_oracle as eo  # noqa: E402
import _exact_oracle as xo  # noqa: E402

from csed_514_project_distributed_training_using_pytorch_amd import ops  # noqa: E402
from csed_514_project_distributed_training_using_pytorch_amd.ops.rng import philox_uniform_reference  # noqa: E402

F64 = torch.float64
NAN, INF = float("nan"), float("inf")


def _close(a, b, tol=1e-12):
    torch.testing.assert_close(a, b, rtol=tol, atol=tol, equal_nan=True)


# ------------------------------------------------------------ torch's float64 ops
@pytest.mark.parametrize("rows,C", [(1, 1), (5, 10), (9, 130)])
def test_log_softmax_and_backward_match_torch(rows, C):
    x = torch.randn(rows, C, dtype=F64, generator=torch.Generator().manual_seed(rows)) * 3
    xr = x.clone().requires_grad_(True)
    y = F.log_softmax(xr, 1)
    _close(eo.log_softmax_ref(x), y.detach())
    dy = eo.int_grads(rows, C)
    y.backward(dy)
    _close(eo.log_softmax_bwd_ref(dy, y.detach()), xr.grad)


def test_log_softmax_inf_and_shift():
    x = torch.tensor([[0.0, -INF, 1.0, -INF], [2.0, 2.0, -INF, -INF]], dtype=F64)
    y = eo.log_softmax_ref(x)
    _close(y, F.log_softmax(x, 1))
    assert torch.equal(y.isinf(), x.isinf()) and not y.isnan().any()
    _close(y[1, :2], torch.full((2,), -np.log(2.0), dtype=F64))
    base = torch.randn(3, 10, dtype=F64)
    _close(eo.log_softmax_ref(base + 80), eo.log_softmax_ref(base), 1e-10)
    # the bound's scale runs over finite entries only: max |x| + |lse|
    assert float(eo.fwd_bound(x, 1.0)[1]) == eo.U * (2.0 + 2.0 + np.log(2.0))
    # a -inf log-prob passes dy through unchanged
    dy = torch.tensor([[1.0, -3.0, 2.0, 4.0]], dtype=F64)
    dx = eo.log_softmax_bwd_ref(dy, y[:1])
    assert dx[0, 1] == -3.0 and dx[0, 3] == 4.0


@pytest.mark.parametrize("reduction", ["none", "mean", "sum"])
@pytest.mark.parametrize("rows,C", [(1, 1), (7, 10), (257, 33)])
def test_nll_and_fused_match_torch(rows, C, reduction):
    g = torch.Generator().manual_seed(rows + C)
    z = (torch.randn(rows, C, dtype=F64, generator=g) * 3).requires_grad_(True)
    t = eo.targets(rows, C)
    logp = F.log_softmax(z, 1)
    logp.retain_grad()
    loss = F.nll_loss(logp, t, reduction=reduction)
    lp_ref, loss_ref = eo.lsm_nll_ref(z.detach(), t, reduction)
    _close(lp_ref, logp.detach())
    _close(loss_ref, loss.detach())
    _close(eo.nll_ref(logp.detach(), t, reduction), loss.detach())
    gout = eo.int_gout(rows, reduction).view(loss.shape)
    loss.backward(gout)
    _close(eo.nll_bwd_ref(gout, t, C, reduction), logp.grad)
    _close(eo.lsm_nll_bwd_ref(gout, logp.detach(), t, reduction), z.grad)


def test_correct_ref_lowest_index_wins():
    lp = torch.tensor([[0.0, 0.0, -1.0],    # tie 0/1 -> 0
                       [-2.0, 0.0, 0.0],    # tie 1/2 -> 1
                       [-1.0, -1.0, -1.0],  # all equal -> 0
                       [-5.0, -4.0, -3.0]], dtype=F64)
    assert eo.correct_ref(lp, torch.tensor([0, 1, 0, 2])) == 4
    assert eo.correct_ref(lp, torch.tensor([1, 2, 1, 2])) == 1
    assert eo.correct_ref(lp, torch.tensor([2, 0, 2, 0])) == 0
    x = torch.randn(50, 7, dtype=F64)  # tie-free: torch's argmax
    t = torch.randint(0, 7, (50,))
    assert eo.correct_ref(x, t) == int((x.argmax(1) == t).sum())


@pytest.mark.parametrize("k,shape", [(2, (2, 3, 7, 9)), (3, (2, 3, 7, 10)), (2, (1, 2, 34, 34))])
def test_pool_matches_torch_on_tie_free_data(k, shape):
    N, C, H, W = shape
    x = torch.randperm(N * C * H * W).to(F64).view(shape) - 300.0  # (distinct values, both signs)
    xr = x.clone().requires_grad_(True)
    pooled, flat = F.max_pool2d(xr, k, return_indices=True)
    y = F.relu(pooled)
    out, idx = eo.pool_fwd_ref(x, k)
    assert torch.equal(out, y.detach())
    PH, PW = H // k, W // k
    hh, ww = flat // W, flat % W
    ph = torch.arange(PH).view(1, 1, PH, 1)
    pw = torch.arange(PW).view(1, 1, 1, PW)
    assert torch.equal(idx.long(), (hh - ph * k) * k + (ww - pw * k))
    dy = xo.grads(torch.Generator().manual_seed(1), y.shape)
    y.backward(dy)
    assert torch.equal(eo.unpool_ref(dy, idx, out, k, shape), xr.grad)
    scale = torch.tensor([0.0, 2.0] * 3)[:N * C]
    assert torch.equal(eo.pool_fwd_ref(x, k, scale)[0], out * scale.view(N, C, 1, 1))
    if k == 2 and H % 2 == 0 and W % 2 == 0:
        assert torch.equal(eo.unpool_ref(dy, idx, out, 2, shape, scale), xo.unpool_ref(dy, idx, out, scale))
        assert torch.equal(out, xo.pool_ref(x)[0]) and torch.equal(idx, xo.pool_ref(x)[1])


def test_pool_hand_cases():
    def one(vals, k=2, scale=None):
        o, i = eo.pool_fwd_ref(torch.tensor(vals, dtype=F64).view(1, 1, k, k), k, scale)
        return o.item(), i.item()

    assert one([1, 3, 3, 2]) == (3.0, 1)            # tie: first of positions 1, 2
    assert one([5, 5, 5, 5]) == (5.0, 0)
    assert one([-3, -1, -2, -1]) == (0.0, 1)        # all negative: 0 out, argmax still recorded (first -1)
    assert one([-0.0, 0.0, -1, 0.0]) == (0.0, 0)    # zeros of both signs tie: the first
    o, i = one([NAN, 7, 1, 2])
    assert np.isnan(o) and i == 0
    o, i = one([9, 7, NAN, 2])
    assert np.isnan(o) and i == 2
    o, i = one([9, NAN, 1, NAN])                    # torch's rule: the last NaN
    assert np.isnan(o) and i == 3
    o, i = one([9, 7, NAN, 2], scale=torch.tensor([0.0]))
    assert np.isnan(o)                              # NaN * 0
    assert one([1, 2, 3, 4, 9, 5, 6, 9, 0], k=3) == (9.0, 4)
    assert one([-2, 3, 1, 0], scale=torch.tensor([-2.0])) == (-6.0, 1)   # relu before the scale
    assert one([-2, -3, -1, -5], scale=torch.tensor([-2.0]))[0] == 0.0
    # torch names the same element for a window with NaNs
    x = torch.tensor([9, NAN, 1, NAN], dtype=F64).view(1, 1, 2, 2)
    assert F.max_pool2d(x, 2, return_indices=True)[1].item() == 3
    # floor: a 3 x 5 plane has one 2 x 2 row of two windows; the border gets no gradient
    x = torch.arange(15, dtype=F64).view(1, 1, 3, 5)
    o, i = eo.pool_fwd_ref(x, 2)
    assert o.flatten().tolist() == [6.0, 8.0] and i.flatten().tolist() == [3, 3]
    dx = eo.unpool_ref(torch.tensor([[[[2.0, 3.0]]]]), i, o, 2, (1, 1, 3, 5))
    assert dx.flatten().tolist() == [0, 0, 0, 0, 0, 0, 2, 0, 3, 0, 0, 0, 0, 0, 0]


def test_max_pool2d_relu_cpu_fallback_is_the_kernels_definition():
    """relu(max_pool(x)) * s, not relu(max_pool(x * s)): they differ for a negative scale."""
    x = eo.pool_input(2, (2, 3, 7, 9), "ties").float()
    for scale in (torch.tensor([0.0, 2.0, 0.0, 2.0, 2.0, 0.0]), torch.tensor([-2.0, 1.0, -1.0, 2.0, 0.0, -3.0])):
        want = eo.pool_fwd_ref(x, 2, scale)[0]
        assert torch.equal(ops.max_pool2d_relu(x, 2, scale).to(F64), want)
    assert (want < 0).any()
    assert torch.equal(ops.max_pool2d_relu(x, 3).to(F64), eo.pool_fwd_ref(x, 3)[0])


def test_keep_scale_and_masks():
    idx = np.arange(1000)
    u = philox_uniform_reference(eo.DROP_SEED, 7 + (3 << 20), idx)
    assert np.array_equal(eo.keep_ref(eo.DROP_SEED, 7, 3, idx, 0.3), u >= np.float32(0.3))
    assert np.array_equal(eo.keep_ref(eo.DROP_SEED, 7, None, idx, 0.3), eo.keep_ref(eo.DROP_SEED, 7, 0, idx, 0.3))
    assert not np.array_equal(eo.keep_ref(eo.DROP_SEED, 7, 3, idx, 0.3), eo.keep_ref(eo.DROP_SEED, 7, 0, idx, 0.3))
    assert not np.array_equal(eo.keep_ref(eo.DROP_SEED, 7, 3, idx, 0.3), philox_uniform_reference(eo.DROP_SEED, 7 + (3 << 16), idx) >= 0.3)
    assert eo.keep_ref(1, 0, None, idx, 0.0).all() and not eo.keep_ref(1, 0, None, idx, 1.0).any()
    assert abs(eo.keep_ref(1, 0, None, np.arange(100000), 0.3).mean() - 0.7) < 0.01
    # the scales: fp32 1 / (1 - p), 0 at p >= 1 (the ones the GPU cases state)
    assert eo.DROP_PS == (0.0, 0.3, 0.5, 1.0)
    assert eo.dropout_scale(0.0) == 1 and eo.dropout_scale(0.5) == 2 and eo.dropout_scale(1.0) == 0
    s = eo.dropout_scale(0.3)
    assert s.dtype == np.float32 and s == np.float32(1) / (np.float32(1) - np.float32(0.3))
    # dropout_ref: channel mode shares a draw per `inner` elements; values are x * scale
    x = eo.drop_input(70 * 35, torch.float32)
    y, keep = eo.dropout_ref(x, 35, 0.5, 5, 0, None)
    per = keep.view(70, 35)
    assert torch.equal(per, per[:, :1].expand(70, 35)) and 10 < int(per[:, 0].sum()) < 60
    assert torch.equal(per[:, 0], torch.from_numpy(eo.keep_ref(5, 0, None, np.arange(70), 0.5)))
    assert torch.equal(y, torch.where(keep, x * 2, torch.zeros(())))
    assert torch.equal(eo.dropout_ref(x, 0, 0.0, 5, 0, None)[0], x)
    assert not eo.dropout_ref(x, 0, 1.0, 5, 0, None)[0].any()
    m = eo.channel_mask_ref(257, 0.3, 5, 7, 3)
    assert m.dtype == torch.float32 and set(m.tolist()) == {0.0, float(s)}
    assert torch.equal(m != 0, torch.from_numpy(eo.keep_ref(5, 7, 3, np.arange(257), 0.3)))


def test_gate_bwd_ref_hand_case():
    dout = torch.tensor([3.0, 3.0, 3.0, 3.0, 3.0, -2.0])
    y = torch.tensor([0.0, -0.0, NAN, -1.0, 0.5, 4.0])
    assert eo.gate_bwd_ref(dout, y, 2.0).tolist() == [0.0, 0.0, 0.0, 0.0, 6.0, -4.0]
    s = eo.GATE_SCALES["sinv0.7"]
    assert s == float(np.float32(1 / 0.7)) and eo.GATE_SCALES["s1"] == 1.0 and eo.GATE_SCALES["s2"] == 2.0
    got = eo.gate_bwd_ref(dout.bfloat16(), y.bfloat16(), s)
    assert got.dtype == torch.bfloat16 and got[4] == torch.tensor(float(np.float32(3) * np.float32(s))).bfloat16()
    assert torch.equal(eo.gate_bwd_ref(dout, y, 2.0).to(F64), xo.gate_ref(dout, y, 2.0))


@pytest.mark.parametrize("elems", eo.GN_ELEMS)
def test_gather_normalize_ref(elems):
    src, idx, labels = eo.gather_input(elems)
    for cursor in eo.GN_CURSORS:
        img, rows = eo.gather_normalize_ref(src, idx, cursor, eo.GN_B, eo.GN_MEAN, eo.GN_STD, torch.float32)
        base = 0 if cursor is None else cursor * eo.GN_B
        assert rows.tolist() == list(eo.GN_IDX[base:base + eo.GN_B])
        plain = (src[rows].reshape(eo.GN_B, -1).to(F64) / 255 - eo.GN_MEAN) / eo.GN_STD
        # fp32 constants: scale carries 3 roundings (1/std, 1/255, their product) on a product <= 3.25, shift 3
        # on 0.43, and the result one of half an ulp below 4: (9.75 + 1.3 + 2) u
        torch.testing.assert_close(img.to(F64), plain, rtol=0, atol=13.05 * eo.U)
        # exact: every byte's value is the rational fma rounded once to fp32
        for b in (0, 1, 127, 255):
            want = np.float32(eo.normalize_exact(b, eo.GN_MEAN, eo.GN_STD))
            hit = src[rows].reshape(eo.GN_B, -1) == b
            assert (img[hit] == float(want)).all()
    assert len(eo.GN_IDX) >= 3 * eo.GN_B + 1 and max(eo.GN_IDX) < eo.GN_ROWS
    assert len(set(eo.GN_IDX[:3])) < 3 and len(set(eo.GN_IDX[6:9])) < 3  # repeated, unordered indices
    if elems == 784:
        for r in range(eo.GN_ROWS):
            assert len(set(src[r].tolist())) == 256


def test_gather_normalize_fma_is_exact_in_float64():
    scale, shift = eo.normalize_constants(eo.GN_MEAN, eo.GN_STD)
    assert scale.dtype == np.float32 and shift.dtype == np.float32
    for b in range(256):
        exact = eo.normalize_exact(b, eo.GN_MEAN, eo.GN_STD)
        assert Fraction(float(b) * float(scale) + float(shift)) == exact  # float64 holds it: one rounding follows


# ------------------------------------------------- preconditions of the exact cases
def test_exact_nll_cases_stay_below_2_24():
    for rows in eo.NLL_ROWS:
        for C in eo.NLL_COLS:
            lp, t = eo.int_logp(rows, C)
            assert torch.equal(lp, lp.round()) and lp.min() >= -64 and lp.max() <= 0
            assert xo.round_trips(lp, torch.float32)
            assert float(lp.abs().sum()) < xo.TWO24  # (any partial sum of any subset, in any order)
            assert int(t.min()) >= 0 and int(t.max()) < C
            if rows >= 3 and C > 1:  # planted ties that include the target's class, won and lost
                is_max = lp == lp.max(1, keepdim=True).values
                tied = torch.arange(rows) % 3 == 0  # (the planted rows; others may tie by chance, below 0)
                assert bool((is_max.sum(1)[tied] > 1).all()) and bool(is_max[tied, t[tied]].all())
                first = torch.where(is_max, torch.arange(C).expand_as(lp), torch.full((rows, C), C)).min(1).values
                if rows >= 255:
                    assert (first[tied] == t[tied]).any() and (first[tied] != t[tied]).any()
            for red in eo.RED:
                g = eo.int_gout(rows, red)
                assert torch.equal(g, g.round()) and xo.round_trips(g, torch.float32)
                # the float64 oracle rounds to the value one fp32 divide gives
                want = eo.nll_bwd_ref(g, t, C, red)
                if red == "mean":
                    assert want[0, t[0]].float().item() == float(-eo.div32(g[0].item(), rows))
                    total = eo.nll_ref(lp, t, "sum")
                    assert eo.nll_ref(lp, t, "mean").float().item() == float(eo.div32(total.item(), rows))


def test_exact_inputs_round_trip_through_their_dtypes():
    for dt in eo.DTYPES:
        for rows, C in ((9, 130), (5, 65)):
            assert xo.round_trips(eo.int_grads(rows, C), dt)
            assert float(eo.int_grads(rows, C).abs().sum(1).max()) < xo.TWO24
        for k, shape in eo.POOL_SHAPES:
            for kind in eo.POOL_KINDS:
                x = eo.pool_input(k, shape, kind)
                fin = torch.nan_to_num(x, nan=0.0)
                assert xo.round_trips(fin, dt) and torch.equal(fin, fin.round()) and fin.abs().max() <= 4
                if kind.startswith("nan"):
                    per_window = eo._windows(x, k).isnan().sum(-1)
                    assert per_window.max() == 1 and per_window.sum() >= 1  # (one NaN a window: no rule needed)
                if kind == "ties" and shape[2] * shape[3] > 4:
                    w = eo._windows(x, k)
                    assert ((w == w.max(-1, keepdim=True).values).sum(-1) > 1).float().mean() > 0.2
                if kind == "negwin":
                    assert (eo._windows(x, k).max(-1).values < 0).any()
                if kind == "negzero":
                    assert torch.signbit(x[x == 0]).any() and (~torch.signbit(x[x == 0])).any()
            s = eo.pool_scale(shape, "scale02")
            assert set(s.tolist()) <= {0.0, 2.0}
        for n in eo.GATE_NS:
            dout, y = eo.gate_input(n, dt, dt, True)
            assert torch.equal(dout.to(F64), dout.to(F64).round()) and dout.to(F64).abs().max() <= 4
            if n > 8:
                assert y.isnan().any() and (y == 0).sum() >= 2 and torch.signbit(y[2]) and (y < 0).any() and (y > 0).any()
    # the shifted log-softmax rows are exact in fp32: the expected answer is the unshifted one's
    for kind in ("up", "down"):
        x, base = eo.logits(9, 130, torch.float32, kind)
        assert torch.equal(x.to(F64), base + (eo.SHIFT if kind == "up" else -eo.SHIFT))
    x, _ = eo.logits(9, 130, torch.bfloat16, "inf")
    assert bool((x.isinf().any(1) & ~x.isinf().all(1)).all())
    x, _ = eo.logits(3, 2, torch.float16, "inf")
    assert bool((x.isinf().any(1) & ~x.isinf().all(1)).all())
    assert not (eo.drop_input(4099, torch.bfloat16) == 0).any()
