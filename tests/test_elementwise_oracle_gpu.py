"""csrc/kernels/elementwise.hip against tests/_elementwise_oracle.py, kernel by kernel through the raw
``torch.ops.csed.*`` ops: each kernel as a function of its own inputs, at the shapes where its loops, blocks and
dtypes take another path.  Every output buffer is pre-filled with NaN (0xFF for argmax bytes), so an element the
kernel does not write fails.  The exact cases are torch.equal over all elements; the log-softmax family carries the
bounds the oracle's docstring derives (no element is skipped or masked; planted -inf entries are asserted exactly).
Each test prints the error it measured before it asserts (``pytest -s``).  1882 cases, 4.5 s on an MI355X.
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _elementwise_oracle as eo  # noqa: E402
from _elementwise_oracle import DTYPES, F64, RED, U, dt_name  # noqa: E402

from csed_514_project_distributed_training_using_pytorch_amd import ops  # noqa: E402
from csed_514_project_distributed_training_using_pytorch_amd.ops import _native, rng  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
NAN = float("nan")
_CACHE: dict = {}
_WORST: dict = {}  # largest error seen per kernel, in units of its bound's scale (printed once, at the end)

dtypes = pytest.mark.parametrize("dt", DTYPES, ids=dt_name)
reductions = pytest.mark.parametrize("red", list(RED))


@pytest.fixture(scope="module", autouse=True)
def _module():
    _native.require()
    yield
    _CACHE.clear()
    for k, v in sorted(_WORST.items()):
        print(f"\n[elementwise oracle] {k}: largest error {v:.3f} units")


def _cached(key, make):
    if key not in _CACHE:
        _CACHE[key] = make()
    return _CACHE[key]


def _o():
    return torch.ops.csed


def _nan(shape, dt):
    return torch.full(tuple(shape), NAN, device=DEV, dtype=dt)


def _dev_off(v):
    return None if v is None else torch.tensor([v], device=DEV, dtype=torch.long)


def _equal(got: torch.Tensor, want: torch.Tensor, what: str) -> None:
    """Same dtype, same shape, same values everywhere; NaNs at the same positions."""
    got = got.detach().cpu()
    assert got.dtype == want.dtype and got.shape == want.shape, f"{what}: {got.dtype} {tuple(got.shape)}"
    if got.is_floating_point():
        assert torch.equal(got.isnan(), want.isnan()), f"{what}: NaN at {torch.nonzero(got.isnan() != want.isnan())[:5].tolist()}"
        got, want = torch.nan_to_num(got, nan=0.0), torch.nan_to_num(want, nan=0.0)
    if torch.equal(got, want):
        return
    bad = torch.nonzero(got != want)
    first = "; ".join(f"{tuple(i.tolist())}: expected {want[tuple(i)].item()} got {got[tuple(i)].item()}" for i in bad[:5])
    raise AssertionError(f"{what}: {bad.shape[0]} of {got.numel()} elements differ; first {first}")


def _within(got: torch.Tensor, ref64: torch.Tensor, scale64: torch.Tensor, c: float, name: str, what: str) -> None:
    """|got - ref| <= c * u * scale at every element (fp32 outputs); records the largest error in units of u * scale."""
    got = got.detach().cpu().to(F64)
    assert not got.isnan().any(), f"{what}: NaN (an element not written?)"
    inf = ref64.isinf()
    assert torch.equal(got[inf], ref64[inf]), f"{what}: the -inf entries"
    err = torch.where(inf, torch.zeros((), dtype=F64), (got - ref64).abs())
    units = err / (U * scale64.expand_as(err))
    worst = float(units.max())
    _WORST[name] = max(_WORST.get(name, 0.0), worst)
    print(f"{what}: {worst:.3f} units (bound {c})")
    assert worst <= c, f"{what}: {worst:.3f} units of u * scale at {tuple(torch.nonzero(units == units.max())[0].tolist())}, bound {c}"


def _stored_within(got: torch.Tensor, ref64: torch.Tensor, scale64: torch.Tensor, c: float, name: str, what: str) -> None:
    """got lies in [round(ref - b), round(ref + b)], b = c * u * scale: an fp32 value within b of ref, stored in got's
    dtype.  For fp32 outputs also records the error in units of u * scale."""
    dt = got.dtype
    got = got.detach().cpu().to(F64)
    assert not got.isnan().any(), f"{what}: NaN (an element not written?)"
    b = (c * U * scale64).expand_as(ref64)
    lo, hi = eo.half_ulp_interval(ref64, b, dt)
    if dt == torch.float32:
        sc = scale64.expand_as(ref64)  # (a zero scale: the value must be exact)
        units = torch.where(sc > 0, (got - ref64).abs() / (U * sc).clamp_min(1e-300),
                            torch.where(got != ref64, float("inf"), 0.0).to(F64))
        _WORST[name] = max(_WORST.get(name, 0.0), float(units.max()))
        print(f"{what}: {float(units.max()):.3f} units (bound {c})")
    bad = torch.nonzero((got < lo) | (got > hi))
    assert bad.shape[0] == 0, (f"{what}: {bad.shape[0]} elements outside the bound; first {tuple(bad[0].tolist())}: "
                               f"got {got[tuple(bad[0])].item()!r}, expected {ref64[tuple(bad[0])].item()!r}")


# ---------------------------------------------------------------- 1. log_softmax_fwd
def _lsm_cases(kinds_of):
    """dtype x kind x rows x C; "inf" (some, not all, entries of a row -inf) needs at least two columns"""
    for dt in DTYPES:
        for kind in kinds_of(dt):
            for rows in eo.LSM_ROWS:
                for C in eo.LSM_COLS:
                    if not (kind == "inf" and C == 1):
                        yield pytest.param(dt, kind, rows, C, id=f"{dt_name(dt)}-{kind}-rows{rows}-C{C}")


@pytest.mark.parametrize("dt,kind,rows,C", list(_lsm_cases(
    lambda dt: ("randn", "inf") + (("up", "down") if dt == torch.float32 else ()))))
def test_log_softmax_fwd(dt, kind, rows, C):
    x, x64 = eo.logits(rows, C, dt, kind)
    want = eo.log_softmax_ref(x64)  # (up / down: of the unshifted rows)
    y = _nan((rows, C), torch.float32)
    _o().log_softmax_fwd(x.to(DEV), y)
    _within(y, want, eo.fwd_scale(x.to(F64)), eo.C_FWD, "log_softmax_fwd",
            f"log_softmax_fwd {dt_name(dt)} {kind} {rows}x{C}")


# ---------------------------------------------------------------- 2. log_softmax_bwd
@pytest.mark.parametrize("dt,kind,rows,C", list(_lsm_cases(lambda dt: ("randn", "inf"))))
def test_log_softmax_bwd(dt, kind, rows, C):
    _, x64 = eo.logits(rows, C, torch.float32, kind)
    y = eo.log_softmax_ref(x64).to(torch.float32)  # (the oracle's log-probs, rounded to fp32: the kernel's input)
    dy = eo.int_grads(rows, C)
    want = eo.log_softmax_bwd_ref(dy, y.to(F64))
    dx = _nan((rows, C), dt)
    _o().log_softmax_bwd(dy.to(DEV, torch.float32), y.to(DEV), dx)
    what = f"log_softmax_bwd {dt_name(dt)} {kind} {rows}x{C}"
    _stored_within(dx, want, dy.abs() + dy.sum(1, keepdim=True).abs(), eo.C_BWD, "log_softmax_bwd", what)
    hole = y.isinf()
    assert torch.equal(dx.cpu()[hole].to(F64), eo.expected(dy, dt)[hole].to(F64)), f"{what}: dx == dy where y is -inf"


# ----------------------------------------------------------------------- 3. nll_fwd
@pytest.mark.parametrize("want_correct", [True, False], ids=["correct", "nocorrect"])
@reductions
@pytest.mark.parametrize("C", eo.NLL_COLS, ids=lambda c: f"C{c}")
@pytest.mark.parametrize("rows", eo.NLL_ROWS, ids=lambda r: f"rows{r}")
def test_nll_fwd(rows, C, red, want_correct):
    lp, t = _cached(("nll", rows, C), lambda: eo.int_logp(rows, C))
    n = rows if red == "none" else 1
    buf = _nan((n + 1,), torch.float32)  # (one guard element behind the output)
    correct = torch.full((1,), -7, device=DEV, dtype=torch.long)
    _o().nll_fwd(lp.to(DEV, torch.float32), t.to(DEV), buf[:n], RED[red], correct if want_correct else None)
    what = f"nll_fwd {rows}x{C} {red}"
    assert buf[n:].isnan().all(), f"{what}: wrote behind its output"
    if red == "mean":
        want = torch.tensor([float(eo.div32(eo.nll_ref(lp, t, "sum").item(), rows))], dtype=torch.float32)
    else:
        want = eo.nll_ref(lp, t, red).to(torch.float32).view(n)
    _equal(buf[:n], want, what)
    assert correct.item() == (eo.correct_ref(lp, t) if want_correct else -7), f"{what}: correct = {correct.item()}"


# ----------------------------------------------------------------------- 4. nll_bwd
@reductions
@pytest.mark.parametrize("C", eo.NLL_COLS, ids=lambda c: f"C{c}")
@pytest.mark.parametrize("rows", eo.NLL_ROWS, ids=lambda r: f"rows{r}")
def test_nll_bwd(rows, C, red):
    t = eo.targets(rows, C)
    g = eo.int_gout(rows, red)
    d = _nan((rows, C), torch.float32)
    _o().nll_bwd(g.to(DEV, torch.float32), t.to(DEV), d, RED[red])
    if red == "mean":  # one correctly rounded fp32 divide
        want = torch.zeros(rows, C, dtype=torch.float32)
        want[torch.arange(rows), t] = -float(eo.div32(g.item(), rows))
    else:
        want = eo.nll_bwd_ref(g, t, C, red).to(torch.float32)
    _equal(d, want, f"nll_bwd {rows}x{C} {red}")


# ------------------------------------------------------------------- 5. lsm_nll_fwd
@reductions
@pytest.mark.parametrize("C", eo.NLL_COLS, ids=lambda c: f"C{c}")
@pytest.mark.parametrize("rows", eo.FUSED_ROWS, ids=lambda r: f"rows{r}")
@dtypes
def test_lsm_nll_fwd(dt, rows, C, red):
    z, z64 = eo.logits(rows, C, dt)
    t = eo.targets(rows, C)
    logp_ref, loss_ref = eo.lsm_nll_ref(z64, t, red)
    n = rows if red == "none" else 1
    logp, out = _nan((rows, C), torch.float32), _nan((n,), torch.float32)
    _o().lsm_nll_fwd(z.to(DEV), t.to(DEV), logp, out, RED[red])
    what = f"lsm_nll_fwd {dt_name(dt)} {rows}x{C} {red}"
    scale = eo.fwd_scale(z64)  # [rows, 1]
    _within(logp, logp_ref, scale, eo.C_FWD, "lsm_nll_fwd", what + " logp")
    if red == "none":
        _within(out, loss_ref, scale.view(rows), eo.C_FWD, "lsm_nll_fwd", what + " losses")
        return
    v = eo.nll_ref(logp_ref, t, "none")
    bound = float(eo.fwd_bound(z64).sum()) + eo.tree_sum_bound(rows, v)
    if red == "mean":
        bound /= rows
    err = abs(float(out.item()) - float(loss_ref))
    print(f"{what}: loss error {err:.3e}, bound {bound:.3e}")
    assert np.isfinite(out.item()) and err <= bound, f"{what}: loss {out.item()!r}, expected {float(loss_ref)!r}, bound {bound:.3e}"


# ------------------------------------------------------------------- 6. lsm_nll_bwd
@reductions
@pytest.mark.parametrize("C", eo.NLL_COLS, ids=lambda c: f"C{c}")
@pytest.mark.parametrize("rows", eo.FUSED_ROWS, ids=lambda r: f"rows{r}")
@dtypes
def test_lsm_nll_bwd(dt, rows, C, red):
    _, z64 = eo.logits(rows, C, torch.float32)
    t = eo.targets(rows, C)
    logp = eo.log_softmax_ref(z64).to(torch.float32)
    g = eo.int_gout(rows, red)
    want = eo.lsm_nll_bwd_ref(g, logp.to(F64), t, red)
    dz = _nan((rows, C), dt)
    _o().lsm_nll_bwd(g.to(DEV, torch.float32), logp.to(DEV), t.to(DEV), dz, RED[red])
    _stored_within(dz, want, eo._row_grad(g, rows, red).abs(), eo.C_BWD, "lsm_nll_bwd",
                   f"lsm_nll_bwd {dt_name(dt)} {rows}x{C} {red}")


# -------------------------------------------------------------- 7. maxpool_relu_fwd
pool_shapes = pytest.mark.parametrize("k,shape", eo.POOL_SHAPES, ids=[eo.pool_id(k, s) for k, s in eo.POOL_SHAPES])


@pytest.mark.parametrize("sc", ["noscale", "scale02"])
@pytest.mark.parametrize("kind", eo.POOL_KINDS)
@pool_shapes
@dtypes
def test_maxpool_relu_fwd(dt, k, shape, kind, sc):
    def make():
        x, scale = eo.pool_input(k, shape, kind), eo.pool_scale(shape, sc)
        return (x, scale) + eo.pool_fwd_ref(x, k, scale)

    x, scale, want, widx = _cached(("pool", k, shape, kind, sc), make)
    out = _nan(want.shape, dt)
    idx = torch.full(want.shape, 0xFF, device=DEV, dtype=torch.uint8)
    _o().maxpool_relu_fwd(x.to(DEV, dt), out, idx, None if scale is None else scale.to(DEV, torch.float32), k)
    what = f"maxpool_relu_fwd {dt_name(dt)} {eo.pool_id(k, shape)} {kind} {sc}"
    _equal(out, eo.expected(want, dt), what + " out")
    _equal(idx, widx, what + " idx")


# -------------------------------------------------------------- 8. maxpool_relu_bwd
def _pool_bwd_dtypes():
    for dt in DTYPES:
        yield pytest.param(dt, dt, id=dt_name(dt))
    for dt in DTYPES[:2]:
        yield pytest.param(torch.float32, dt, id=f"f32-into-{dt_name(dt)}")


@pytest.mark.parametrize("k,shape", [(2, (1, 2, 34, 34)), (3, (2, 3, 7, 10))], ids=["k2-plane289", "k3-2x3x7x10"])
@pytest.mark.parametrize("ddt,dt", list(_pool_bwd_dtypes()))
def test_maxpool_relu_bwd(ddt, dt, k, shape):
    def make():
        g = eo._gen(k, 19)
        x, scale = eo.pool_input(k, shape, "ties"), eo.pool_scale(shape, "scale02")
        out, idx = eo.pool_fwd_ref(x, k, scale)
        dyp = eo.ints(g, out.shape, -4, 4, zero_share=0.25)
        return out, idx, dyp, scale, eo.unpool_ref(dyp, idx, out, k, shape, scale)

    out, idx, dyp, scale, want = _cached(("unpool", k, shape), make)
    dx = _nan(shape, dt)
    _o().maxpool_relu_bwd(dyp.to(DEV, ddt), out.to(DEV, dt), idx.to(DEV), scale.to(DEV, torch.float32), dx, k)
    _equal(dx, eo.expected(want, dt), f"maxpool_relu_bwd {dt_name(ddt)}->{dt_name(dt)} {eo.pool_id(k, shape)}")


# ------------------------------------------------------------------- 9. dropout_fwd
drop_cross = [pytest.mark.parametrize("dev", eo.DROP_DEVS, ids=lambda v: "nodev" if v is None else f"dev{v}"),
              pytest.mark.parametrize("off", eo.DROP_OFFSETS, ids=lambda v: f"off{v}"),
              pytest.mark.parametrize("p", eo.DROP_PS, ids=eo.p_id)]
DROP_SHAPES = [pytest.param(n, 0, id=f"total{n}") for n in eo.DROP_TOTALS] + \
              [pytest.param(eo.DROP_CHANNELS * i, i, id=f"ch70-inner{i}") for i in eo.DROP_INNERS]


def _cross(f):
    for m in drop_cross:
        f = m(f)
    return f


@_cross
@pytest.mark.parametrize("n,inner", DROP_SHAPES)
@dtypes
def test_dropout_fwd(dt, n, inner, p, off, dev):
    x = _cached(("dropx", n, dt), lambda: eo.drop_input(n, dt))
    want, keep = eo.dropout_ref(x, inner, p, eo.DROP_SEED, off, dev)
    y = _nan((n,), dt)
    _o().dropout_fwd(x.to(DEV), y, inner, p, eo.DROP_SEED, off, _dev_off(dev))
    what = f"dropout_fwd {dt_name(dt)} n{n} inner{inner} p{p} off{off} dev{dev}"
    got = y.cpu()
    assert not got.isnan().any(), f"{what}: NaN"
    if p < 1:
        assert torch.equal(got != 0, keep), f"{what}: mask differs at {torch.nonzero((got != 0) != keep)[:5].flatten().tolist()}"
    _equal(y, want, what)
    if p == 1:
        assert not got.any(), f"{what}: p = 1 must give zeros"
    if p == 0:
        bits = torch.int32 if dt == torch.float32 else torch.int16
        assert torch.equal(got.view(bits), x.view(bits)), f"{what}: p = 0 must pass the input through bit for bit"


# ---------------------------------------- 10. ops.dropout / dropout2d / dropout2d_scale
@pytest.mark.parametrize("step", [None, 5], ids=["nostep", "step5"])
def test_dropout_wrappers_offsets_and_backward(step):
    st = rng.default_state
    saved = (st._seed, st._offset, st.device_step)
    try:
        rng.manual_seed(0xC0FFEE)
        st.device_step = _dev_off(step)
        seed, p = st.seed, 0.5
        x1 = eo.drop_input(64, torch.float32).to(DEV).requires_grad_(True)
        x2 = eo.drop_input(64 * 9, torch.bfloat16).view(4, 16, 3, 3).to(DEV).requires_grad_(True)
        y1 = ops.dropout(x1, p, True)             # host offset 0
        y2 = ops.dropout2d(x2, p, True)           # 1
        s3 = ops.dropout2d_scale(4, 16, p, DEV)   # 2
        keeps = [torch.from_numpy(eo.keep_ref(seed, o, step, np.arange(64), p)) for o in range(3)]
        assert torch.equal(y1.detach().cpu() != 0, keeps[0])
        assert torch.equal(y2.detach().cpu() != 0, keeps[1].view(4, 16, 1, 1).expand(4, 16, 3, 3))
        assert torch.equal(s3.cpu() != 0, keeps[2])
        _equal(y1, eo.dropout_ref(x1.detach().cpu(), 0, p, seed, 0, step)[0], "ops.dropout")
        _equal(y2, eo.dropout_ref(x2.detach().cpu(), 9, p, seed, 1, step)[0], "ops.dropout2d")
        _equal(s3, eo.channel_mask_ref(64, p, seed, 2, step), "ops.dropout2d_scale")
        for a in range(3):
            for b in range(a + 1, 3):
                assert not torch.equal(keeps[a], keeps[b]), f"calls {a} and {b} drew the same mask"
        if step is not None:  # the masks follow the step tensor's value
            assert not torch.equal(keeps[0], torch.from_numpy(eo.keep_ref(seed, 0, None, np.arange(64), p)))
        # the backward regenerates the forward's mask
        g1 = eo.drop_input(64, torch.float32)
        g2 = eo.drop_input(64 * 9, torch.bfloat16).view(4, 16, 3, 3)
        y1.backward(g1.to(DEV))
        y2.backward(g2.to(DEV))
        _equal(x1.grad, eo.dropout_ref(g1, 0, p, seed, 0, step)[0], "ops.dropout backward")
        _equal(x2.grad, eo.dropout_ref(g2, 9, p, seed, 1, step)[0], "ops.dropout2d backward")
    finally:
        st._seed, st._offset, st.device_step = saved


# ------------------------------------------------------------------ 11. channel_mask
@_cross
@pytest.mark.parametrize("n", eo.MASK_NS, ids=lambda n: f"n{n}")
def test_channel_mask(n, p, off, dev):
    sc = _nan((n,), torch.float32)
    _o().channel_mask(sc, p, eo.DROP_SEED, off, _dev_off(dev))
    _equal(sc, eo.channel_mask_ref(n, p, eo.DROP_SEED, off, dev), f"channel_mask n{n} p{p} off{off} dev{dev}")


# ---------------------------------------------------------------------- 12. gate_bwd
@pytest.mark.parametrize("s", list(eo.GATE_SCALES))
@pytest.mark.parametrize("n", eo.GATE_NS, ids=lambda n: f"n{n}")
@pytest.mark.parametrize("ydt", DTYPES, ids=lambda d: "y" + dt_name(d))
@dtypes
def test_gate_bwd(dt, ydt, n, s):
    dout, y = eo.gate_input(n, dt, ydt, exact=s != "sinv0.7")
    dx = _nan((n,), dt)
    _o().gate_bwd(dout.to(DEV), y.to(DEV), dx, eo.GATE_SCALES[s])
    _equal(dx, eo.gate_bwd_ref(dout, y, eo.GATE_SCALES[s]), f"gate_bwd {dt_name(dt)} y{dt_name(ydt)} n{n} {s}")


# -------------------------------------------------------------- 13. gather_normalize
@pytest.mark.parametrize("labels", [True, False], ids=["labels", "nolabels"])
@pytest.mark.parametrize("cursor", eo.GN_CURSORS, ids=lambda c: "nocursor" if c is None else f"cursor{c}")
@pytest.mark.parametrize("elems", eo.GN_ELEMS, ids=lambda e: f"elems{e}")
@dtypes
def test_gather_normalize(dt, elems, cursor, labels):
    src, idx, lab_src = eo.gather_input(elems)
    want, rows = eo.gather_normalize_ref(src, idx, cursor, eo.GN_B, eo.GN_MEAN, eo.GN_STD, dt)
    out = _nan((eo.GN_B, elems), dt)
    lab = torch.full((eo.GN_B,), -7, device=DEV, dtype=torch.long)
    _o().gather_normalize(src.to(DEV), idx.to(DEV), _dev_off(cursor), eo.GN_B, eo.GN_MEAN, eo.GN_STD, out,
                          lab if labels else None, lab_src.to(DEV) if labels else None)
    what = f"gather_normalize {dt_name(dt)} elems{elems} cursor{cursor}"
    _equal(out, want, what)
    _equal(lab, lab_src[rows] if labels else torch.full((eo.GN_B,), -7, dtype=torch.long), what + " labels")
