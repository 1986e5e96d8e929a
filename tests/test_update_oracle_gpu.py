"""csed::lenet_update, lenet_sgd_kernel and sgd_flat against an fp64 oracle of their own operation
(tests/_update_oracle.py; tests/test_update_oracle_cpu.py ties that oracle to the layout header).

The update kernel gets synthetic slabs written through the layout contract and must return exactly
the plain sums (integer inputs: every fp32 sum is exact in any order) or the sums within the bound of
an fp32 summation (real inputs), at every FC configuration the per-rank batch selects: one wave per
tile with the small-batch K-steps (B <= 32), one 64-sample chunk, two (<= 128), 2 / 4 / 8 waves per
tile with the LDS combine (129.. / 257.. / 513..) and the split-K slices (> 1024 with the scratch).
Everything a launch must not use holds NaN (stale samples from B on, slab padding, slab floats past
the layout's span): the readers mask or never read them, so no NaN may reach the output.  The SGD tests
run every hyperparameter of torch.optim.SGD through all three kernels that implement its rule, one fp64
reference step from the kernel's own state per launch.  No test here runs lenet_train."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _update_oracle as orc  # noqa: E402
from _update_oracle import LR, NP, SGD_TABLE  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
DTYPES = [torch.bfloat16, torch.float16, torch.float32]
U = 2.0 ** -24  # relative error of one fp32 rounding
SENTINEL = 1234.5  # momentum buffer content where no kernel may touch it
SEGMENTS = (("conv1.weight", 0, 250), ("conv1.bias", 250, 260), ("conv2.weight", 260, 5260), ("conv2.bias", 5260, 5280),
            ("fc1.weight", 5280, 21280), ("fc1.bias", 21280, 21330), ("fc2.weight", 21330, 21830),
            ("fc2.bias", 21830, 21840))
_ENGINES: dict = {}


def _dt(dtype) -> str:
    return str(dtype).replace("torch.", "")


def _build_engine(dtype, B, loopback_world=0):
    from csed_514_project_distributed_training_using_pytorch_amd.data.mnist import MNISTData
    from csed_514_project_distributed_training_using_pytorch_amd.engine.fused import FusedLeNetTrainer
    from csed_514_project_distributed_training_using_pytorch_amd.models import Net

    # (the images' content is irrelevant here: no test runs a training kernel)
    data = MNISTData(torch.zeros((B, 28, 28), dtype=torch.uint8), torch.zeros(B, dtype=torch.long), True)
    torch.manual_seed(1)
    return FusedLeNetTrainer(Net().to(DEV), data, lr=LR, momentum=0.5, global_batch=B, compute_dtype=dtype,
                             drop_p=0.0, loopback_world=loopback_world)


def _engine(dtype, B):
    """One engine per (dtype, batch) for the whole file: B = 1024 (a 256-row slab, 1024 vector samples;
    smaller shapes are launched on it with update_args(B=, grid=)) and B = 2051 (the split-K scratch)."""
    if (dtype, B) not in _ENGINES:
        _ENGINES[(dtype, B)] = _build_engine(dtype, B)
    return _ENGINES[(dtype, B)]


@pytest.fixture(scope="module", autouse=True)
def _drop_engines():
    yield
    _ENGINES.clear()


def _counters(eng) -> tuple:
    return (int(eng.cursor.item()), int(eng.rng_offset.item()), int(eng.step_count.item()), int(eng.ticket.item()))


def _where(bad: torch.Tensor) -> str:
    """Which parameters fail, per layer (so a failure names the kernel role behind it)."""
    parts = [f"{name} {int(bad[lo:hi].sum())}/{hi - lo} (first {lo + int(torch.nonzero(bad[lo:hi])[0])})"
             for name, lo, hi in SEGMENTS if bad[lo:hi].any()]
    return "; ".join(parts)


def _assert_exact(got: torch.Tensor, want: torch.Tensor, what: str) -> None:
    got, want = got.cpu(), want.cpu()
    if not torch.equal(got, want):
        bad = ~(got == want)  # (NaN counts as a mismatch)
        i = int(torch.nonzero(bad)[0])
        raise AssertionError(f"{what}: {_where(bad)}; element {i}: got {got[i].item()!r}, want {want[i].item()!r}")


def _assert_within(got: torch.Tensor, want: torch.Tensor, bound: torch.Tensor, what: str) -> None:
    err = (got.cpu().double() - want).abs()
    bad = ~(err <= bound)  # (NaN counts as a violation)
    if bad.any():
        i = int(torch.nonzero(bad)[0])
        ratio = (err / bound.clamp_min(1e-300))[~torch.isnan(err)].max().item()
        raise AssertionError(f"{what}: {_where(bad)}; element {i}: got {got[i].item()!r}, want {want[i].item()!r}, "
                             f"bound {bound[i].item():.3e}; worst error / bound {ratio:.3f}")


def _fc_counters_zero(eng) -> bool:
    cnt = eng.fc_counters()  # (the layout's fc_counters_off / fc_tiles: pinned by tests/test_launch_args_cpu.py)
    return cnt.numel() == 88 and not bool(cnt.any().item())


def _reduce(eng, B, grid, out, grad_post, fc_split=None, exchange=False, with_loss=True):
    # scale_in_kernel=False: the update kernel applies grad_post whatever the engine's dtype
    torch.ops.csed.lenet_update(*eng.update_args("reduce", B=B, grid=grid, grad=out, exchange=exchange,
                                                 grad_scale=grad_post, scale_in_kernel=False, fc_split=fc_split,
                                                 with_loss=with_loss))


# (engine batch, B, grid, fc_split): one workgroup per sample; the split step's 4 workgroups per sample;
# multi-sample grids; the split-K engine with its scratch (2051 = two slices of 1056 + 995), without it,
# and with it at a batch that takes one slice
SHAPES_EXACT = ([(1024, B, B, None) for B in (1, 3, 8, 9, 16, 17, 31, 32, 33, 63, 64, 65, 100, 128, 129, 200, 256)]
                + [(1024, B, 4 * B, None) for B in (1, 8, 24, 64)]
                + [(1024, B, g, None) for B, g in ((100, 7), (257, 256), (500, 256), (512, 256), (513, 256),
                                                   (777, 256), (1000, 256), (1024, 256))]
                + [(2051, 2051, 256, None), (2051, 2051, 256, False), (2051, 1100, 256, None)])


def _shape_id(s) -> str:
    return f"B{s[1]}-grid{s[2]}" + ("" if s[0] == 1024 else f"-eng{s[0]}") + ("-nosplit" if s[3] is False else "")


# ------------------------------------------------------------------ (a) reduce mode, exact
@pytest.mark.parametrize("shape", SHAPES_EXACT, ids=_shape_id)
@pytest.mark.parametrize("dtype", DTYPES, ids=_dt)
def test_reduce_integer_inputs_exact(dtype, shape):
    """Integer slabs and vectors (exact in bf16 / fp16; every partial sum an integer below 2^24, so the
    fp32 result does not depend on the summation order), NaN in everything the launch must not use, the
    output prefilled with NaN: all 21,840 gradients equal the fp64 reference bit for bit.  grad_post 1
    and 1/64 scale exactly; 1/100 is one fp32 multiply of the exact sum.  The same launches fold the loss
    partials (nparts = grid, up to 256) into a preset accumulator, and a reduce advances no counter."""
    eng_b, B, grid, fc_split = shape
    eng = _engine(dtype, eng_b)
    for k, gp in enumerate((1.0, 1.0 / 64, 1.0 / 100)):
        inp = orc.make_inputs(B, grid, dtype, "int", 1000 * k + 7 * B + grid)
        ref = orc.reference(inp, B, grid, gp)
        want = ref.sums.float() * torch.tensor(gp, dtype=torch.float32)  # one fp32 multiply
        if k < 2:
            assert torch.equal(want.double(), ref.grad)  # (a power-of-two scale: the reference itself)
        orc.fill(eng, inp, B, grid, poison=True)
        acc0 = torch.tensor([3.0 + k, 5.0])
        eng.loss_acc.copy_(acc0)
        out = torch.full((NP,), float("nan"), device=DEV)
        before = _counters(eng)
        _reduce(eng, B, grid, out, gp, fc_split=fc_split)
        torch.cuda.synchronize()
        _assert_exact(out, want, f"{_dt(dtype)} B {B} grid {grid} grad_post {gp}")
        assert torch.equal(eng.loss_acc.cpu(), acc0 + inp.loss.sum(0)), "loss partials"
        assert _counters(eng) == before, "a reduce advances neither cursor, Philox offset, step nor ticket"
        if eng.fc_part is not None:
            assert _fc_counters_zero(eng), "split-K arrival counters not back at zero"


# ------------------------------------------------------------------ (b) reduce mode, real values
SHAPES_REAL = [(1024, 8, 8), (1024, 33, 33), (1024, 64, 64), (1024, 100, 7), (1024, 200, 200), (1024, 500, 256),
               (1024, 777, 256), (2051, 2051, 256)]
# the FC configuration each of these batches stands for: (waves per tile, split-K slices) of the launch's plan
FC_CONFIG = {8: (1, 1), 33: (1, 1), 64: (1, 1), 100: (1, 1), 200: (2, 1), 500: (4, 1), 777: (8, 1), 2051: (8, 2)}


@pytest.mark.parametrize("shape", SHAPES_REAL, ids=lambda s: f"B{s[1]}-grid{s[2]}")
@pytest.mark.parametrize("dtype", DTYPES, ids=_dt)
def test_reduce_real_inputs_within_fp32_summation_bound(dtype, shape):
    """Standard-normal slabs and vectors (the vectors rounded to the compute dtype for bf16 / fp16, full
    fp32 for the fp32 layout -- not representable in 16 bits, so an operand truncated on its way into
    the MFMA fails here), poisoned like the exact test, one shape per FC configuration.

    Bound, derived (u = 2^-24): every gradient is a sum of n addends a_k.  Conv addends are fp32 slab
    values, 16-bit fc addends products of two bf16 / fp16 values (8 + 8 or 11 + 11 significand bits:
    exact in fp32): exactly represented, so an fp32 sum of them in ANY order (any tree over slab rows,
    K-steps, waves, slices) carries at most n - 1 roundings, each of a partial sum no larger than
    S = sum |a_k|:  |error| <= (n - 1) u S to first order.  fp32 fc addends are products of two fp32
    values: one more rounding of each product (none if the MFMA fuses), at most u S in all.  grad_post
    is one more multiply: u |sum| <= u S.  Together (n + 1) u S |grad_post|; the test allows
    (n + 2) u S |grad_post|, the slack covering the second-order terms ((n + 1) u < 2.5e-4 here)."""
    eng_b, B, grid = shape
    eng = _engine(dtype, eng_b)
    plan = eng.update_plan(eng.update_args("reduce", B=B, grid=grid, grad=eng.flat.data, exchange=False))  # (grad: any tensor)
    assert (plan.waves_per_tile, plan.slices) == FC_CONFIG[B] and not plan.error
    gp = 1.0 / B
    inp = orc.make_inputs(B, grid, dtype, "real", 31 * B + grid)
    ref = orc.reference(inp, B, grid, gp)
    orc.fill(eng, inp, B, grid, poison=True)
    out = torch.full((NP,), float("nan"), device=DEV)
    _reduce(eng, B, grid, out, gp, with_loss=False)
    torch.cuda.synchronize()
    bound = (ref.n.double() + 2) * U * ref.sabs * abs(ref.grad_post)
    _assert_within(out, ref.grad, bound, f"{_dt(dtype)} B {B} grid {grid}")
    if eng.fc_part is not None:
        assert _fc_counters_zero(eng)


# ------------------------------------------------------------------ SGD helpers
def _set_hyper(eng, mom, damp, wd, nesterov) -> None:
    eng.lr, eng.momentum, eng.dampening, eng.weight_decay, eng.nesterov = LR, mom, damp, wd, nesterov


def _reset_state(eng, mom) -> None:
    """Known parameters, a zero momentum buffer (a sentinel where the rule has none), step counter 0."""
    gen = torch.Generator().manual_seed(11)
    eng.flat.data.copy_(torch.randn(NP, generator=gen) * 0.25)
    eng.repack()
    eng.momentum_buf.fill_(SENTINEL if mom == 0 else 0.0)
    eng.step_count.zero_()
    eng.ticket.zero_()


def _check_sgd_step(eng, g, p0, m0, step0, hyper, what) -> None:
    """After one SGD launch from (p0, m0) at step counter ``step0`` with gradient g (fp64): parameters and
    buffer against one fp64 reference step within sgd_bounds (derived there: 8 u on the magnitudes that
    enter the rule), the no-momentum and first-step rules, and the 16-bit weight images."""
    mom, damp, wd, nesterov = hyper
    first = step0 == 0 and damp != 0
    p_ref, m_ref = orc.sgd_reference(p0, m0, g, first, LR, mom, damp, wd, nesterov)
    bm, bp = orc.sgd_bounds(p0, m0 if mom != 0 else torch.zeros_like(m0), g, LR, mom, wd)
    _assert_within(eng.flat.data, p_ref, bp, f"{what}: parameters")
    if mom == 0:
        assert torch.equal(eng.momentum_buf.cpu(), m0), f"{what}: momentum 0 must leave the buffer untouched"
    else:
        _assert_within(eng.momentum_buf, m_ref, bm, f"{what}: momentum buffer")
    if first:
        # torch's first step stores buf = g + wd p, not (1 - damp) times it: the two differ by far more
        # than the bound, so the check above can tell them apart
        gj = g + orc.f32(wd) * p0.double()
        assert torch.equal(m_ref, gj) and bool((orc.f32(damp) * gj.abs() > 4 * bm).any())
    if not eng.fp32:
        w = eng.wimg.clone()
        eng.repack()
        nbad = int((w != eng.wimg).sum().item())
        assert nbad == 0, f"{what}: {nbad} weight-image elements are not the repacked new parameters"


# ------------------------------------------------------------------ (c) SGD inside the update kernel
STEP_SHAPES = ([(torch.bfloat16, 1024, 8, 8), (torch.bfloat16, 1024, 64, 64), (torch.bfloat16, 1024, 200, 200),
                (torch.bfloat16, 2051, 2051, 256), (torch.float16, 1024, 64, 64), (torch.float32, 1024, 64, 64)])


@pytest.mark.parametrize("hyper", SGD_TABLE, ids=lambda h: "m%g-d%g-wd%g-%s" % (h[0], h[1], h[2], "nag" if h[3] else "std"))
@pytest.mark.parametrize("case", STEP_SHAPES, ids=lambda c: f"{_dt(c[0])}-B{c[2]}")
def test_step_mode_sgd_matches_fp64_rule(case, hyper):
    """mode="step": integer slabs with grad_post = 1/64, so the gradient the kernel applies is known
    exactly; three consecutive launches with fresh inputs, each checked against one fp64 step from the
    kernel's own state (the bound does not compound).  The shapes reach every finisher: the conv role,
    the float4 row-layout fc1 tiles (finish_param4), the per-element bias-column and fc2 tiles, the
    finish after the multi-wave combine (B = 200) and by the last-arriving split-K slice (B = 2051)."""
    dtype, eng_b, B, grid = case
    eng = _engine(dtype, eng_b)
    mom = hyper[0]
    _set_hyper(eng, *hyper)
    _reset_state(eng, mom)
    gp = 1.0 / 64
    for step in range(3):
        inp = orc.make_inputs(B, grid, dtype, "int", 100 * step + B + int(1000 * mom))
        ref = orc.reference(inp, B, grid, gp)
        assert torch.equal(ref.grad.float().double(), ref.grad)  # exact in fp32
        orc.fill(eng, inp, B, grid, poison=True)
        acc0 = torch.tensor([2.0, 1.0])
        eng.loss_acc.copy_(acc0)
        p0, m0 = eng.flat.data.cpu().clone(), eng.momentum_buf.cpu().clone()
        cur, rng, cnt, _ = _counters(eng)
        assert cnt == step
        torch.ops.csed.lenet_update(*eng.update_args("step", B=B, grid=grid, exchange=False, grad_scale=gp,
                                                     scale_in_kernel=False))
        torch.cuda.synchronize()
        what = f"{_dt(dtype)} B {B} step {step} (momentum, dampening, weight_decay, nesterov) = {hyper}"
        assert _counters(eng) == (cur + 1, rng + 1, cnt + 1, 0), f"{what}: cursor / Philox offset / step + 1, ticket 0"
        assert torch.equal(eng.loss_acc.cpu(), acc0 + inp.loss.sum(0)), f"{what}: loss partials"
        if eng.fc_part is not None:
            assert _fc_counters_zero(eng), f"{what}: split-K arrival counters"
        _check_sgd_step(eng, ref.grad, p0, m0, cnt, hyper, what)


# ------------------------------------------------------------------ (d) SGD from a reduced gradient
@pytest.mark.parametrize("hyper", SGD_TABLE, ids=lambda h: "m%g-d%g-wd%g-%s" % (h[0], h[1], h[2], "nag" if h[3] else "std"))
@pytest.mark.parametrize("dtype", DTYPES, ids=_dt)
def test_apply_mode_sgd_matches_fp64_rule(dtype, hyper):
    """mode="apply" (lenet_sgd_kernel): a real-valued gradient of 21,840 floats, three launches, the same
    per-step reference and bound.  The loss accumulator is not this launch's.  The device cursor and
    Philox offset are: "apply" is the launch of the three-kernel step (reduce, all-reduce, apply) that
    advances them, by exactly one -- and a launch that is given neither leaves both alone."""
    eng = _engine(dtype, 1024)
    mom = hyper[0]
    _set_hyper(eng, *hyper)
    _reset_state(eng, mom)
    gen = torch.Generator().manual_seed(23)
    acc0 = torch.tensor([7.0, 9.0])
    eng.loss_acc.copy_(acc0)
    for step in range(3):
        g = torch.randn(NP, generator=gen) * 0.1
        p0, m0 = eng.flat.data.cpu().clone(), eng.momentum_buf.cpu().clone()
        cur, rng, cnt, _ = _counters(eng)
        args = eng.update_args("apply", grad=g.to(DEV))
        assert args.cursor is eng.cursor and args.rng_offset is eng.rng_offset and args.loss_acc is None
        if step == 1:
            args = args._replace(cursor=None, rng_offset=None)
        torch.ops.csed.lenet_update(*args)
        torch.cuda.synchronize()
        what = f"{_dt(dtype)} apply step {step} (momentum, dampening, weight_decay, nesterov) = {hyper}"
        adv = 0 if step == 1 else 1
        assert _counters(eng) == (cur + adv, rng + adv, cnt + 1, 0), what
        assert torch.equal(eng.loss_acc.cpu(), acc0), f"{what}: loss accumulator touched"
        _check_sgd_step(eng, g.double(), p0, m0, cnt, hyper, what)


# ------------------------------------------------------------------ (e) sgd_flat
@pytest.mark.parametrize("hyper", SGD_TABLE, ids=lambda h: "m%g-d%g-wd%g-%s" % (h[0], h[1], h[2], "nag" if h[3] else "std"))
@pytest.mark.parametrize("gscale", [1.0, 1.0 / 64], ids=["scale1", "scale64th"])
@pytest.mark.parametrize("n", [21840, 1027, 3])
def test_sgd_flat_matches_fp64_rule(n, gscale, hyper):
    """csed::sgd_flat (float4 body + scalar tail: n = 1027 has both, n = 3 the tail alone): three launches,
    one fp64 reference step each from the kernel's own state, within sgd_bounds.  Its first-step rule is
    step[0] == 0 (the buffer is not read then: it holds NaN here); momentum 0 leaves the buffer alone."""
    mom, damp, wd, nesterov = hyper
    gen = torch.Generator().manual_seed(n + 5)
    p = (torch.randn(n, generator=gen) * 0.25).to(DEV)
    buf = torch.full((n,), SENTINEL if mom == 0 else float("nan"), device=DEV)
    step = torch.zeros(1, dtype=torch.long, device=DEV)
    ticket = torch.zeros(1, dtype=torch.int32, device=DEV)
    for k in range(3):
        g = torch.randn(n, generator=gen)
        p0, m0 = p.cpu().clone(), buf.cpu().clone()
        torch.ops.csed.sgd_flat(p, g.to(DEV), buf, LR, mom, damp, wd, nesterov, gscale, step, ticket)
        torch.cuda.synchronize()
        assert step.item() == k + 1 and ticket.item() == 0
        ge = g.double() * orc.f32(gscale)
        mz = torch.zeros(n) if (k == 0 or mom == 0) else m0  # (no buffer enters the first step)
        p_ref, m_ref = orc.sgd_reference(p0, mz, ge, k == 0, LR, mom, damp, wd, nesterov)
        bm, bp = orc.sgd_bounds(p0, mz, ge, LR, mom, wd)
        err_p = (p.cpu().double() - p_ref).abs()
        assert bool((err_p <= bp).all()), f"n {n} step {k} {hyper}: parameters, worst error / bound {(err_p / bp).max():.3f}"
        if mom == 0:
            assert torch.equal(buf.cpu(), m0), "momentum 0 must leave the buffer untouched"
        else:
            err_m = (buf.cpu().double() - m_ref).abs()
            assert bool((err_m <= bm).all()), f"n {n} step {k} {hyper}: buffer, worst error / bound {(err_m / bm).max():.3f}"


# ------------------------------------------------------------------ (f) loopback exchange
@pytest.mark.parametrize("world,B", [(2, 200), (4, 300), (8, 600)])
def test_loopback_exchange_at_multi_wave_fc_shapes(world, B):
    """The fused exchange runs one FC tile per workgroup with the batch's waves per tile: 2, 4 and 8 here
    (tests/test_exchange_loopback_gpu.py stops at B = 64, one wave).  Integer inputs, poisoned, reduce
    mode with the exchange in loopback: exactly world x the fp64 reference, two rounds (both slot
    parities), no timed-out wait (every wait is bounded by the engine's timeout)."""
    eng = _build_engine(torch.bfloat16, B, loopback_world=world)
    try:
        for rnd in range(2):
            inp = orc.make_inputs(B, eng.grid, torch.bfloat16, "int", 50 * world + rnd)
            ref = orc.reference(inp, B, eng.grid, 1.0)
            orc.fill(eng, inp, B, eng.grid, poison=True)
            out = torch.full((NP,), float("nan"), device=DEV)
            _reduce(eng, B, eng.grid, out, 1.0, exchange=True, with_loss=False)
            torch.cuda.synchronize()
            _assert_exact(out, (ref.sums * world).float(), f"world {world} B {B} round {rnd}")
        assert eng.comm_errors() == 0
    finally:
        eng.close()
