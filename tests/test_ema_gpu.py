"""The device-resident exponential moving average of the weights on the GPU: csed::lenet_update in every
form that applies SGD and lenet_sgd_kernel against an fp64 replay of the rule

    e <- e + (1 - d) (p_new - e)        (fp32, 1 - d formed in fp32 from the float32 d)

stacked on tests/_update_oracle.py's SGD reference, then the engines around them: graph replay, eager
steps and the native executor, the loopback exchange, save / restore, the graph cache and evaluation of
the averaged weights.

Bound of the oracle cases, per element (u = 2^-24, P the parameter bound of sgd_bounds):
|e_kernel - e_fp64| <= (1 - d) P + 4 u (|e_old| + |p_new|) -- the parameter's own error enters scaled by
1 - d, and the kernel rounds p_new - e, 1 - d and one fma, each on a term no larger than |e_old| +
|p_new|: three roundings, the bound gives them 4.

The split-K case needs a forced slice count (CSED_FC_SLICES), which the launcher reads once per process:
it runs this file as a script in a child process."""
import os
import subprocess
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _update_oracle as orc  # noqa: E402
from _update_oracle import LR, NP  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
U = 2.0 ** -24
D = 0.9
HYPER = (0.9, 0.0, 5e-4, True)  # (momentum, dampening, weight_decay, nesterov)
_ENGINES: dict = {}


def _dt(dtype) -> str:
    return str(dtype).replace("torch.", "")


def _build_engine(dtype, B, loopback_world=0):
    from csed_514_project_distributed_training_using_pytorch_amd.data.mnist import MNISTData
    from csed_514_project_distributed_training_using_pytorch_amd.engine.fused import FusedLeNetTrainer
    from csed_514_project_distributed_training_using_pytorch_amd.models import Net

    # (the images' content is irrelevant to the oracle cases: none of them runs a training kernel)
    data = MNISTData(torch.zeros((B, 28, 28), dtype=torch.uint8), torch.zeros(B, dtype=torch.long), True)
    torch.manual_seed(1)
    return FusedLeNetTrainer(Net().to(DEV), data, lr=LR, momentum=0.5, global_batch=B, compute_dtype=dtype,
                             drop_p=0.0, loopback_world=loopback_world)


def _engine(dtype, B=256):
    """One engine per dtype for the oracle cases (a 256-row slab; smaller shapes are launched on it with
    update_args(B=, grid=), as tests/test_update_oracle_gpu.py does)."""
    if (dtype, B) not in _ENGINES:
        _ENGINES[(dtype, B)] = _build_engine(dtype, B)
    return _ENGINES[(dtype, B)]


@pytest.fixture(scope="module", autouse=True)
def _drop_engines():
    yield
    _ENGINES.clear()


def _within(got, want, bound, what):
    err = (got.cpu().double() - want).abs()
    bad = ~(err <= bound)
    if bad.any():
        i = int(torch.nonzero(bad)[0])
        raise AssertionError(f"{what}: {int(bad.sum())} elements, first {i}: got {got[i].item()!r}, want "
                             f"{want[i].item()!r}, bound {bound[i].item():.3e}; worst error / bound "
                             f"{(err / bound.clamp_min(1e-300)).max().item():.3f}")


def ema_reference(e_old, p_new, d):
    """The rule in fp64 from the old average and the (fp64) new parameters; d as the kernel receives it."""
    e = e_old.double()
    return e + (1.0 - orc.f32(d)) * (p_new - e)


def ema_bound(e_old, p_new, p_bound, d):
    return (1.0 - orc.f32(d)) * p_bound + 4 * U * (e_old.double().abs() + p_new.abs())


def _set_state(eng, p, m, e=None):
    eng.flat.data.copy_(p)
    eng.momentum_buf.copy_(m)
    eng.repack()
    eng.step_count.fill_(1)  # (a momentum buffer exists)
    eng.ticket.zero_()
    if e is not None:
        eng.ema.copy_(e)


def _launch(eng, mode_args, pair):
    """One SGD-applying launch: "step", or the "reduce" then "apply" pair of the all-reduce fallback."""
    if pair:
        g = torch.full((NP,), float("nan"), device=DEV)
        torch.ops.csed.lenet_update(*eng.update_args("reduce", grad=g, **mode_args))
        kw = {k: v for k, v in mode_args.items() if k in ("B", "grid")}
        torch.ops.csed.lenet_update(*eng.update_args("apply", grad=g, **kw))
    else:
        torch.ops.csed.lenet_update(*eng.update_args("step", **mode_args))
    torch.cuda.synchronize()


def _check_plan(eng, B, grid, exchange, fc_split, expect):
    plan = eng.update_plan(eng.update_args("step", B=B, grid=grid, exchange=exchange, fc_split=fc_split))
    assert not plan.error
    for k, v in expect.items():
        assert getattr(plan, k) == v, f"plan.{k} = {getattr(plan, k)}, the case is meant for {v}"


def run_oracle_case(eng, B, grid, *, exchange=False, fc_split=None, pair=False, world=1, table=None, expect=None,
                    d=D, seed=0):
    """One SGD-applying launch from filled integer slabs (grad_post 1/64: the gradient the kernel applies is
    exact in fp32, so sgd_bounds holds as derived) with random nonzero parameters, momentum and average:
    the same launch without the average first (parameters, momentum and weight image must then be the same
    bits with it), the average against the fp64 rule, a second launch from the first one's state, and a
    reduce-only launch that must leave the average alone."""
    from csed_514_project_distributed_training_using_pytorch_amd.optim import LRSchedule

    mom, damp, wd, nesterov = HYPER
    eng.lr, eng.momentum, eng.dampening, eng.weight_decay, eng.nesterov = LR, mom, damp, wd, nesterov
    gp = 1.0 / 64
    args = dict(B=B, grid=grid, exchange=exchange, grad_scale=gp, scale_in_kernel=False, fc_split=fc_split)
    gen = torch.Generator().manual_seed(100 + seed)
    p0, m0, e0 = (torch.randn(NP, generator=gen) * s for s in (0.25, 0.1, 0.25))
    try:
        eng.set_lr_schedule(None if table is None else LRSchedule(torch.tensor(table)))
        eng.set_ema(None)
        if expect:
            _check_plan(eng, B, grid, exchange, fc_split, expect)
        inp = orc.make_inputs(B, grid, eng.compute_dtype, "int", 7 * B + grid + seed)
        ref = orc.reference(inp, B, grid, gp)
        g = ref.grad * world  # (a looped-back peer returns this rank's own gradient)
        assert torch.equal(g.float().double(), g)
        orc.fill(eng, inp, B, grid, poison=True)
        # --- without the average
        _set_state(eng, p0, m0)
        _launch(eng, args, pair)
        p_off, m_off, w_off = eng.flat.data.clone(), eng.momentum_buf.clone(), eng.wimg.clone()
        if table is not None:
            eng.lr_schedule.pos.zero_()
        # --- with it: two launches, each against one fp64 step from the kernel's own state
        eng.set_ema(d)
        assert eng.update_args("step", **args).ema is eng.ema and eng.update_args("step", **args).ema_decay == d
        _set_state(eng, p0, m0, e0)
        for k in range(2):
            pk, mk, ek = eng.flat.data.cpu().clone(), eng.momentum_buf.cpu().clone(), eng.ema.cpu().clone()
            lr = LR if table is None else table[min(k, len(table) - 1)]
            _launch(eng, args, pair)
            what = f"{_dt(eng.compute_dtype)} B {B} grid {grid} launch {k}"
            if k == 0:
                assert torch.equal(eng.flat.data, p_off), f"{what}: parameters differ from the launch without ema"
                assert torch.equal(eng.momentum_buf, m_off), f"{what}: momentum differs from the launch without ema"
                assert torch.equal(eng.wimg, w_off), f"{what}: weight image differs from the launch without ema"
            p_ref, _ = orc.sgd_reference(pk, mk, g, False, lr, mom, damp, wd, nesterov)
            _, bp = orc.sgd_bounds(pk, mk, g, lr, mom, wd)
            _within(eng.flat.data, p_ref, bp, f"{what}: parameters")
            _within(eng.ema, ema_reference(ek, p_ref, d), ema_bound(ek, p_ref, bp, d), f"{what}: ema")
            assert not torch.equal(eng.ema.cpu(), ek), f"{what}: the average did not move"
        # --- a reduce-only launch is given no average and touches none
        e2 = eng.ema.clone()
        out = torch.full((NP,), float("nan"), device=DEV)
        rargs = eng.update_args("reduce", grad=out, **args)
        assert rargs.ema is None and rargs.ema_decay == 0.0
        torch.ops.csed.lenet_update(*rargs)
        torch.cuda.synchronize()
        assert torch.equal(eng.ema, e2), "a reduce-only launch changed the average"
        assert eng.comm_errors() == 0
    finally:
        eng.set_ema(None)
        eng.set_lr_schedule(None)


# ------------------------------------------------------------------ oracle cases
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16, torch.float32], ids=_dt)
def test_plain_step_b8(dtype):
    """One workgroup per sample, B = 8 on grid 8: the conv role, the float4 fc1 rows (finish_param4) and the
    per-element bias-column and fc2 tiles (finish_param), in every compute-dtype instantiation."""
    run_oracle_case(_engine(dtype), 8, 8, expect=dict(slices=1, waves_per_tile=1, sched=0, world_bound=0))


def test_split_step_b16_grid64():
    """The split step's slab layout (4 workgroups per sample)."""
    run_oracle_case(_engine(torch.bfloat16), 16, 64, seed=1)


def test_two_waves_per_tile_b129():
    """B = 129: two waves per FC tile, the finish after the LDS combine."""
    run_oracle_case(_engine(torch.bfloat16), 129, 129, seed=2, expect=dict(waves_per_tile=2, slices=1))


def run_split_k_case():
    """Split-K fc gradients at B = 513, the smallest batch a forced slice count applies to (CSED_FC_SLICES=2
    in this process): the tile's last-arriving slice loads p / m / e itself and finishes."""
    eng = _build_engine(torch.bfloat16, 1025)  # (the smallest engine that allocates the split-K scratch)
    run_oracle_case(eng, 513, min(256, eng.grid), seed=3, fc_split=True, expect=dict(slices=2))
    assert not bool(eng.fc_counters().any().item())


def test_split_k_forced_slices_b513():
    env = dict(os.environ, CSED_FC_SLICES="2")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "split-k"], env=env, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0 and "split-k ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


def test_loopback_exchange_world2_b8():
    """The fused exchange (looped back, world 2): the summed gradient is twice the rank's own."""
    eng = _build_engine(torch.bfloat16, 8, loopback_world=2)
    try:
        run_oracle_case(eng, 8, eng.grid, exchange=True, world=2, seed=4, expect=dict(world_bound=2, loopback=1))
    finally:
        eng.close()


def test_scheduled_step():
    """The SCHED instantiation: each launch trains at its own table entry and still averages."""
    run_oracle_case(_engine(torch.bfloat16), 8, 8, table=[0.05, 0.0125], seed=5, expect=dict(sched=1))


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=_dt)
def test_reduce_then_apply_pair(dtype):
    """The all-reduce fallback's launches: "reduce" (no average) then "apply" (lenet_sgd_kernel)."""
    run_oracle_case(_engine(dtype), 8, 8, pair=True, seed=6)


def test_integer_case_is_exact():
    """Integer slabs with grad_post 1/64, integer parameters, momentum and average, lr = 1/16, momentum 0.5,
    d = 0.5: every operation of the SGD rule and of the average is exact in fp32, so both must equal the
    fp64 values bit for bit (a fused or reordered form of the rule gives the same bits here; a wrong one
    does not)."""
    for dtype, B, grid in ((torch.bfloat16, 8, 8), (torch.float32, 8, 8), (torch.bfloat16, 129, 129)):
        eng = _engine(dtype)
        eng.lr, eng.momentum, eng.dampening, eng.weight_decay, eng.nesterov = 1.0 / 16, 0.5, 0.0, 0.0, False
        gen = torch.Generator().manual_seed(B)
        p0, m0, e0 = (torch.randint(-8, 9, (NP,), generator=gen).float() for _ in range(3))
        inp = orc.make_inputs(B, grid, dtype, "int", B + 3)
        ref = orc.reference(inp, B, grid, 1.0 / 64)
        orc.fill(eng, inp, B, grid, poison=True)
        try:
            eng.set_ema(0.5)
            _set_state(eng, p0, m0, e0)
            torch.ops.csed.lenet_update(*eng.update_args("step", B=B, grid=grid, exchange=False, grad_scale=1.0 / 64,
                                                         scale_in_kernel=False))
            torch.cuda.synchronize()
            p_ref, _ = orc.sgd_reference(p0, m0, ref.grad, False, 1.0 / 16, 0.5, 0.0, 0.0, False)
            e_ref = ema_reference(e0, p_ref, 0.5)
            assert torch.equal(eng.flat.data.cpu().double(), p_ref), f"{_dt(dtype)} B {B}: parameters"
            assert torch.equal(eng.ema.cpu().double(), e_ref), f"{_dt(dtype)} B {B}: ema"
        finally:
            eng.set_ema(None)
            eng.lr, eng.momentum = LR, 0.5


# ------------------------------------------------------------------ op rejections
def test_ops_reject_bad_ema():
    eng = _engine(torch.bfloat16)
    base = eng.update_args("step", B=8, grid=8, exchange=False)
    good = torch.zeros(NP, device=DEV)
    bad = [("float32", base._replace(ema=good.double(), ema_decay=0.9)),
           ("one value per parameter", base._replace(ema=torch.zeros(NP - 4, device=DEV), ema_decay=0.9)),
           ("parameters' device", base._replace(ema=torch.zeros(NP), ema_decay=0.9)),
           (r"ema_decay must be in \[0, 1\)", base._replace(ema=good, ema_decay=1.0)),
           (r"ema_decay must be in \[0, 1\)", base._replace(ema=good, ema_decay=-0.1))]
    out = torch.zeros(NP, device=DEV)
    bad.append(("only with apply_sgd", eng.update_args("reduce", B=8, grid=8, grad=out, exchange=False)
                ._replace(ema=good, ema_decay=0.9)))
    p0 = eng.flat.data.clone()
    for msg, args in bad:
        with pytest.raises(RuntimeError, match=msg):
            torch.ops.csed.lenet_update(*args)
    st = torch.classes.csed.LenetStepper()
    with pytest.raises(RuntimeError, match="float32"):
        st.set_update(*base._replace(cursor=eng.cursor, ema=good.double(), ema_decay=0.9))
    torch.cuda.synchronize()
    assert torch.equal(eng.flat.data, p0), "a rejected call launched something"


# ------------------------------------------------------------------ training sequences
ORDER = torch.arange(68).roll(5) % 64  # 8 full steps of 8 and a tail of 4: 9 steps per epoch


def _trainer(loopback_world=0, ema=0.99):
    from csed_514_project_distributed_training_using_pytorch_amd.data.mnist import synthetic_mnist
    from csed_514_project_distributed_training_using_pytorch_amd.engine.fused import FusedLeNetTrainer
    from csed_514_project_distributed_training_using_pytorch_amd.models import Net

    torch.manual_seed(1)
    eng = FusedLeNetTrainer(Net().to(DEV), synthetic_mnist(64, seed=3), lr=0.05, momentum=0.5, global_batch=8,
                            loopback_world=loopback_world)
    if ema is not None:
        eng.set_ema(ema)
    return eng


def _final(eng):
    torch.cuda.synchronize()
    return eng.ema.clone(), eng.flat.data.clone(), eng.momentum_buf.clone()


def _same(a, b, what):
    for name, x, y in zip(("ema", "params", "momentum"), a, b):
        assert torch.equal(x, y), f"{what}: {name} differ in {int((x != y).sum())} elements"


@pytest.fixture(scope="module")
def graph_run():
    """Two epochs (18 steps, two of them tails) replayed from graphs: the reference of the sequence tests."""
    eng = _trainer()
    e_start = eng.ema.clone()
    eng.train_epoch(ORDER)
    mid = _final(eng)
    eng.train_epoch(ORDER)
    out = _final(eng)
    assert eng.tail_size() == 4 and eng.full_steps() == 8
    assert not torch.equal(mid[0], e_start) and not torch.equal(out[0], mid[0]) and not torch.equal(out[0], out[1])
    eng.close()
    return out


def test_graph_replay_equals_eager_and_native_executor(graph_run):
    eager = _trainer()
    for _ in range(2):
        eager.set_epoch_order(ORDER)
        for _ in range(eager.full_steps()):
            eager.step()
        eager._tail_step()
    _same(_final(eager), graph_run, "eager steps vs graph replay")
    eager.close()
    native = _trainer()
    for _ in range(2):
        native.train_epoch(ORDER, use_graph=False)
    assert native._stepper is not None, "the native executor did not run"
    _same(_final(native), graph_run, "native executor vs graph replay")
    native.close()


def test_loopback2_training_equals_world1(graph_run):
    eng = _trainer(loopback_world=2)
    for _ in range(2):
        eng.train_epoch(ORDER)
    assert eng.comm_errors() == 0
    _same(_final(eng), graph_run, "loopback world 2 vs world 1")
    eng.close()


def test_resume_from_state_dicts(graph_run):
    """One epoch, then everything a checkpoint holds (model, optimizer, ema) into a fresh engine, which also
    continues the first one's Philox offset (the dropout masks' position, no part of any file)."""
    from csed_514_project_distributed_training_using_pytorch_amd.models import Net

    a = _trainer()
    a.train_epoch(ORDER)
    torch.cuda.synchronize()
    model_sd = {k: v.detach().cpu().clone() for k, v in a.model.state_dict().items()}
    opt_sd, ema_sd, rng = a.optimizer_state_dict(), a.ema_state_dict(), a.rng_offset.clone()
    a.close()
    ref_net = Net()
    ref_net.load_state_dict(ema_sd)  # (stock load_state_dict: the Net parameter names)
    assert all(v.dtype == torch.float32 and v.device.type == "cpu" for v in ema_sd.values())
    b = _trainer(ema=None)
    b.model.load_state_dict(model_sd)
    b.params_changed()
    b.load_optimizer_state_dict(opt_sd)
    b.set_ema(0.99)
    assert torch.equal(b.ema, b.flat.data), "set_ema starts at a copy of the current parameters"
    b.load_ema_state_dict(ema_sd)
    b.rng_offset.copy_(rng)
    b.train_epoch(ORDER)
    _same(_final(b), graph_run, "resumed vs uninterrupted")
    b.close()


def test_set_ema_drops_captured_graphs():
    eng = _trainer(ema=None)
    eng.set_epoch_order(ORDER)
    eng.run_steps(2)
    eng.stepper()
    assert eng._graphs and eng._stepper is not None
    eng.set_ema(0.99)
    assert not eng._graphs and eng._stepper is None, "set_ema must drop the graphs and the executor"
    e0 = eng.ema.clone()
    eng.run_steps(2)
    torch.cuda.synchronize()
    assert eng._graphs and not torch.equal(eng.ema, e0), "the replayed steps did not move the average"
    eng.set_ema(None)
    assert not eng._graphs and eng._stepper is None and eng.ema is None
    assert eng.update_args("step").ema is None
    eng.close()


def test_evaluate_ema():
    from csed_514_project_distributed_training_using_pytorch_amd.data.mnist import synthetic_mnist

    test = synthetic_mnist(100, seed=5)
    a = _trainer(ema=0.9)
    assert a.evaluate(test, ema=True) == a.evaluate(test), "before any step the average is the parameters"
    a.train_epoch(ORDER)
    torch.cuda.synchronize()
    assert not torch.equal(a.ema, a.flat.data)
    got, raw, logp = a.evaluate(test, ema=True), a.evaluate(test), a.eval_logp(test, ema=True)
    b = _trainer(ema=None)
    b.flat.data.copy_(a.ema)
    b.params_changed()
    assert got == b.evaluate(test), "evaluate(ema=True) is not the evaluation of the averaged parameters"
    assert torch.equal(logp, b.eval_logp(test))
    assert got != raw and a.evaluate(test) == raw, "evaluating the average must not disturb the parameters' image"
    with pytest.raises(RuntimeError, match="set_ema"):
        b.evaluate(test, ema=True)
    a.close()
    b.close()


def test_per_op_optimizer_refuses_ema_on_gpu():
    """csed::sgd_flat keeps no average: a GPU FusedSGD must say so, not average with torch kernels."""
    from csed_514_project_distributed_training_using_pytorch_amd.optim import FusedSGD

    opt = FusedSGD([torch.zeros(8, device=DEV, requires_grad=True)], lr=0.1, momentum=0.5)
    with pytest.raises(NotImplementedError, match="fused engine"):
        opt.set_ema(0.9)
    assert opt.ema_flat is None


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))  # (the package, as pytest finds it)
    assert sys.argv[1:] == ["split-k"] and os.environ.get("CSED_FC_SLICES") == "2"
    run_split_k_case()
    print("split-k ok")
