"""Adam / AdamW on the device (csed::lenet_update_adam): every form of lenet_update that applies the gradient
and lenet_sgd_kernel against the fp64 oracle of tests/_adam_oracle.py within its derived bounds, then the
engine around them: the real train kernel's gradient, graph replay / eager / native executor / reduce-apply
fallback / loopback exchange bit for bit, the torch-compatible state dict, the op's rejections and the
untouched SGD default.

The oracle cases fill integer slabs (tests/_update_oracle.py) with a power-of-two grad_post, so the gradient
the kernel applies is exact in fp32 and equal to the fp64 reference's; each of three consecutive launches is
compared with one oracle step from the kernel's own previous fp32 state, so errors do not compound.  The moving
average is compared with e + (1 - d)(p_new - e) from the kernel's own new parameters: p_new - e, 1 - d and one
fma, three roundings of terms <= |e| + |p_new|, bound 4 u (|e| + |p_new|).

The split-K case needs a forced slice count (CSED_FC_SLICES), which the launcher reads once per process: it
runs this file as a script in a child process."""
import itertools
import os
import subprocess
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _adam_oracle as ado  # noqa: E402
import _update_oracle as orc  # noqa: E402
from _update_oracle import NP  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
U = 2.0 ** -24
LR, BETAS, EPS, WD, D = 1e-3, (0.9, 0.999), 1e-8, 1e-2, 0.9
TABLE = [1e-3, 2.5e-4, 5e-4]
# (AdamW, schedule, moving average)
VARIANTS = list(itertools.product((False, True), (False, True), (False, True)))
_ENGINES: dict = {}


def _dt(dtype) -> str:
    return str(dtype).replace("torch.", "")


def _vid(v) -> str:
    return ("adamw" if v[0] else "adam") + ("-sched" if v[1] else "") + ("-ema" if v[2] else "")


def _build_engine(dtype, B, loopback_world=0):
    from csed_514_project_distributed_training_using_pytorch_amd.data.mnist import MNISTData
    from csed_514_project_distributed_training_using_pytorch_amd.engine.fused import FusedLeNetTrainer
    from csed_514_project_distributed_training_using_pytorch_amd.models import Net

    # (the images' content is irrelevant to the oracle cases: none of them runs a training kernel)
    data = MNISTData(torch.zeros((B, 28, 28), dtype=torch.uint8), torch.zeros(B, dtype=torch.long), True)
    torch.manual_seed(1)
    return FusedLeNetTrainer(Net().to(DEV), data, lr=LR, global_batch=B, compute_dtype=dtype, drop_p=0.0,
                             loopback_world=loopback_world, optimizer="adam", betas=BETAS, eps=EPS, weight_decay=WD)


def _engine(dtype, B=8, loopback_world=0):
    key = (dtype, B, loopback_world)
    if key not in _ENGINES:
        _ENGINES[key] = _build_engine(dtype, B, loopback_world)
    return _ENGINES[key]


@pytest.fixture(scope="module", autouse=True)
def _drop_engines():
    yield
    for eng in _ENGINES.values():
        eng.close()
    _ENGINES.clear()


def _within(got, want, bound, what):
    err = (got.cpu().double() - want).abs()
    bad = ~(err <= bound)  # (NaN counts as a violation)
    if bad.any():
        i = int(torch.nonzero(bad)[0])
        raise AssertionError(f"{what}: {int(bad.sum())} elements, first {i}: got {got[i].item()!r}, want "
                             f"{want[i].item()!r}, bound {bound[i].item():.3e}; worst error / bound "
                             f"{(err / bound.clamp_min(1e-300)).max().item():.3f}")


def _launch(eng, mode_args, pair):
    """One gradient-applying launch: "step", or the "reduce" then "apply" pair of the all-reduce fallback."""
    ops = torch.ops.csed
    if pair:
        g = torch.full((NP,), float("nan"), device=DEV)
        name, args = eng.update_launch("reduce", grad=g, **mode_args)
        assert name == "lenet_update", "the fallback's reduce-only launch stays lenet_update"
        getattr(ops, name)(*args)
        kw = {k: v for k, v in mode_args.items() if k in ("B", "grid")}
        name, args = eng.update_launch("apply", grad=g, **kw)
    else:
        name, args = eng.update_launch("step", **mode_args)
    assert name == "lenet_update_adam" and args.mom == 0.0 and args.adam_v is eng.adam_v
    getattr(ops, name)(*args)
    torch.cuda.synchronize()


def run_oracle_case(eng, B, grid, variant, *, exchange=False, fc_split=None, pair=False, world=1, expect=None, seed=0):
    from csed_514_project_distributed_training_using_pytorch_amd.optim import LRSchedule

    decoupled, sched, ema = variant
    eng.optimizer = "adamw" if decoupled else "adam"
    gp = 1.0 / 64
    args = dict(B=B, grid=grid, exchange=exchange, grad_scale=gp, scale_in_kernel=False, fc_split=fc_split)
    gen = torch.Generator().manual_seed(100 + seed)
    p0, m0, e0 = (torch.randn(NP, generator=gen) * s for s in (0.25, 0.1, 0.25))
    v0 = torch.rand(NP, generator=gen) * 0.01
    v0[::9] = 0.0
    try:
        eng.set_lr_schedule(LRSchedule(torch.tensor(TABLE)) if sched else None)
        eng.set_ema(D if ema else None)
        if expect:
            plan = eng.update_plan(eng.update_args("step", **args))
            assert not plan.error
            for k, want in dict(expect, sched=int(sched)).items():
                assert getattr(plan, k) == want, f"plan.{k} = {getattr(plan, k)}, the case is meant for {want}"
        eng.flat.data.copy_(p0), eng.momentum_buf.copy_(m0), eng.adam_v.copy_(v0)
        if ema:
            eng.ema.copy_(e0)
        eng.repack()
        eng.step_count.zero_(), eng.ticket.zero_()
        for k in range(3):
            inp = orc.make_inputs(B, grid, eng.compute_dtype, "int", 7 * B + grid + seed + 1000 * k)
            g = orc.reference(inp, B, grid, gp).grad * world  # (a looped-back peer returns this rank's own gradient)
            assert torch.equal(g.float().double(), g)
            orc.fill(eng, inp, B, grid, poison=True)
            pk, mk, vk = eng.flat.data.cpu().clone(), eng.momentum_buf.cpu().clone(), eng.adam_v.cpu().clone()
            ek = eng.ema.cpu().clone() if ema else None
            lr = TABLE[k] if sched else LR
            _launch(eng, args, pair)
            what = f"{_dt(eng.compute_dtype)} B {B} grid {grid} {_vid(variant)} launch {k}"
            assert int(eng.step_count.item()) == k + 1 and int(eng.ticket.item()) == 0, what
            hyper = (k + 1, lr, BETAS, EPS, WD, decoupled)
            p_ref, m_ref, v_ref = ado.adam_reference(pk, mk, vk, g, *hyper)
            bm, bv, bp = ado.adam_bounds(pk, mk, vk, g, *hyper)
            _within(eng.momentum_buf, m_ref, bm, f"{what}: exp_avg")
            _within(eng.adam_v, v_ref, bv, f"{what}: exp_avg_sq")
            _within(eng.flat.data, p_ref, bp, f"{what}: parameters")
            assert not torch.equal(eng.flat.data.cpu(), pk), f"{what}: the parameters did not move"
            image = eng.wimg.clone()
            eng.repack()
            assert torch.equal(eng.wimg, image), f"{what}: the weight image is not repack() of the new parameters"
            if ema:
                pn, e = eng.flat.data.cpu().double(), ek.double()
                _within(eng.ema, e + (1.0 - orc.f32(D)) * (pn - e), 4 * U * (e.abs() + pn.abs()), f"{what}: ema")
            if sched:
                assert int(eng.lr_schedule.pos.item()) == k + 1
        if eng.fc_part is not None:
            assert not bool(eng.fc_counters().any().item()), "split-K arrival counters not back at zero"
        assert eng.comm_errors() == 0
    finally:
        eng.set_ema(None)
        eng.set_lr_schedule(None)
        eng.optimizer = "adam"


# ------------------------------------------------------------------ oracle cases
@pytest.mark.parametrize("variant", VARIANTS, ids=_vid)
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16, torch.float32], ids=_dt)
def test_split_step_plain_form_b8(dtype, variant):
    """B = 8 on the split step's grid (4 workgroups per sample): the conv role, the float4 fc1 rows and the
    per-element bias-column and fc2 tiles, in every compute-dtype instantiation."""
    run_oracle_case(_engine(dtype, 32), 8, 32, variant, expect=dict(slices=1, waves_per_tile=1, world_bound=0))


@pytest.mark.parametrize("variant", VARIANTS, ids=_vid)
def test_loopback_exchange_world2_b8(variant):
    """The fused exchange looped back (world 2) with its invariant check: the summed gradient is twice the
    rank's own."""
    eng = _engine(torch.bfloat16, 8, loopback_world=2)
    run_oracle_case(eng, 8, eng.grid, variant, exchange=True, world=2, seed=4, expect=dict(world_bound=2, loopback=1))


@pytest.mark.parametrize("variant", VARIANTS, ids=_vid)
def test_loopback_exchange_idle_waves_b130(variant):
    """B = 130: more than one wave per FC tile, the exchange packing through the idle waves."""
    eng = _engine(torch.bfloat16, 130, loopback_world=2)
    run_oracle_case(eng, 130, eng.grid, variant, exchange=True, world=2, seed=2, expect=dict(world_bound=2, loopback=1))


@pytest.mark.parametrize("variant", VARIANTS, ids=_vid)
def test_apply_from_grad_in_b8(variant):
    """The all-reduce fallback's launches: "reduce" (lenet_update, no optimizer) then "apply" (lenet_sgd_kernel)."""
    run_oracle_case(_engine(torch.bfloat16, 32), 8, 8, variant, pair=True, seed=6)


def run_split_k_case():
    """Split-K fc gradients at B = 1025 (CSED_FC_SLICES=2 in this process): the tile's last-arriving slice
    loads p / m / v / e itself and finishes."""
    eng = _build_engine(torch.bfloat16, 1025)
    for variant in VARIANTS:
        run_oracle_case(eng, 1025, min(256, eng.grid), variant, seed=3, fc_split=True, expect=dict(slices=2))
    eng.close()


def test_split_k_finish_path_b1025():
    env = dict(os.environ, CSED_FC_SLICES="2")
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "split-k"], env=env, capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0 and "split-k ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


# ------------------------------------------------------------------ through the real train kernel


def _trainer(B=8, dtype=torch.bfloat16, loopback_world=0, optimizer="adam", wd=0.0, **kw):
    from csed_514_project_distributed_training_using_pytorch_amd.data.mnist import synthetic_mnist
    from csed_514_project_distributed_training_using_pytorch_amd.engine.fused import FusedLeNetTrainer
    from csed_514_project_distributed_training_using_pytorch_amd.models import Net

    torch.manual_seed(1)
    return FusedLeNetTrainer(Net().to(DEV), synthetic_mnist(64 * max(1, B // 8), seed=3), lr=LR, global_batch=B,
                             compute_dtype=dtype, loopback_world=loopback_world, optimizer=optimizer, weight_decay=wd, **kw)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=_dt)
def test_step_applies_adam_to_the_train_kernels_gradient(dtype):
    """gradient() then step() from the same state and cursor (a reduce-only launch advances neither cursor nor
    Philox offset, so both see the same batch and masks): the step's p, m, v are the oracle's on that gradient."""
    eng = _trainer(dtype=dtype, optimizer="adamw", wd=WD)
    eng.set_epoch_order(torch.arange(64))
    for t in (1, 2):
        pk, mk, vk = eng.flat.data.cpu().clone(), eng.momentum_buf.cpu().clone(), eng.adam_v.cpu().clone()
        g = eng.gradient().cpu().double()
        assert bool(g.abs().sum() > 0)
        eng.step()
        torch.cuda.synchronize()
        hyper = (t, LR, BETAS, EPS, WD, True)
        ref, bounds = ado.adam_reference(pk, mk, vk, g, *hyper), ado.adam_bounds(pk, mk, vk, g, *hyper)
        for name, got, want, b in zip(("exp_avg", "exp_avg_sq", "parameters"), (eng.momentum_buf, eng.adam_v, eng.flat.data),
                                      (ref[1], ref[2], ref[0]), bounds):
            _within(got, want, b, f"{_dt(dtype)} step {t}: {name}")
    assert int(eng.step_count.item()) == 2
    eng.close()


# ------------------------------------------------------------------ bitwise structure
def _final(eng):
    torch.cuda.synchronize()
    return eng.flat.data.clone(), eng.momentum_buf.clone(), eng.adam_v.clone(), eng.wimg.clone(), eng.step_count.clone()


def _same(a, b, what):
    for name, x, y in zip(("params", "exp_avg", "exp_avg_sq", "weight image", "step"), a, b):
        assert torch.equal(x, y), f"{what}: {name} differ in {int((x != y).sum())} elements"


@pytest.fixture(scope="module", params=[8, 64], ids=lambda b: f"B{b}")
def graph_run(request):
    """Eight Adam steps replayed from a graph: the reference of the sequence tests."""
    B = request.param
    eng = _trainer(B)
    start = eng.flat.data.clone()
    eng.set_epoch_order(torch.arange(8 * B))
    eng.run_steps(8)
    out = _final(eng)
    assert eng._graphs and int(out[4].item()) == 8 and not torch.equal(out[0], start)
    names = [n for n, _ in eng._step_launches()]
    assert names == ["lenet_train", "lenet_update_adam"]
    eng.close()
    return B, out


def test_graph_replay_equals_eager_and_native_executor(graph_run):
    B, want = graph_run
    eager = _trainer(B)
    eager.set_epoch_order(torch.arange(8 * B))
    for _ in range(8):
        eager.step()
    _same(_final(eager), want, "eager steps vs graph replay")
    eager.close()
    native = _trainer(B)
    native.set_epoch_order(torch.arange(8 * B))
    native.run_steps(8, use_graph=False)
    assert native._stepper is not None, "the native executor did not run"
    _same(_final(native), want, "native executor vs graph replay")
    native.close()


def test_reduce_apply_fallback_equals_one_kernel_step(graph_run):
    B, want = graph_run
    eng = _trainer(B)
    eng.set_epoch_order(torch.arange(8 * B))
    ops = torch.ops.csed
    g = torch.empty(NP, device=DEV)
    for _ in range(8):
        ops.lenet_train(*eng.train_args(stage_next=True))
        for mode in ("reduce", "apply"):
            name, args = eng.update_launch(mode, grad=g)
            assert name == ("lenet_update" if mode == "reduce" else "lenet_update_adam")
            getattr(ops, name)(*args)
    _same(_final(eng), want, "reduce -> apply vs the one-kernel step")
    eng.close()


def test_loopback2_training_equals_world1(graph_run):
    B, want = graph_run
    eng = _trainer(B, loopback_world=2)
    eng.set_epoch_order(torch.arange(8 * B))
    eng.run_steps(8)
    assert eng.comm_errors() == 0
    _same(_final(eng), want, "loopback world 2 vs world 1")
    eng.close()


# ------------------------------------------------------------------ state dict
def test_state_dict_loads_into_torch_and_round_trips():
    from csed_514_project_distributed_training_using_pytorch_amd.models import Net

    a = _trainer()
    a.set_epoch_order(torch.arange(64))
    assert a.optimizer_state_dict()["state"] == {}
    a.run_steps(3)
    torch.cuda.synchronize()
    sd = a.optimizer_state_dict()
    ref = torch.optim.Adam(Net().parameters())
    assert list(sd["param_groups"][0]) == list(ref.state_dict()["param_groups"][0])
    ref.load_state_dict(sd)
    st = ref.state_dict()["state"][0]
    assert st["step"].dtype == torch.float32 and float(st["step"]) == 3.0 and st["step"].dim() == 0
    assert torch.equal(st["exp_avg_sq"], a.flat.view(a.adam_v, 0).cpu())
    model_sd = {k: v.detach().cpu().clone() for k, v in a.model.state_dict().items()}
    rng, cur = a.rng_offset.clone(), a.cursor.clone()
    a.run_steps(3)
    want = _final(a)
    a.close()
    b = _trainer()
    b.set_epoch_order(torch.arange(64))
    b.model.load_state_dict(model_sd)
    b.params_changed()
    b.load_optimizer_state_dict(sd)
    assert int(b.step_count.item()) == 3
    b.rng_offset.copy_(rng), b.cursor.copy_(cur)
    b._stage_current()
    b.run_steps(3)
    _same(_final(b), want, "resumed vs uninterrupted")
    sgd = _trainer(optimizer="sgd", momentum=0.5)
    with pytest.raises(ValueError, match="not Adam's"):
        b.load_optimizer_state_dict(sgd.optimizer_state_dict())
    w = _trainer(optimizer="adamw")
    with pytest.raises(ValueError, match="AdamW"):
        b.load_optimizer_state_dict(w.optimizer_state_dict())
    assert w.optimizer_state_dict()["param_groups"][0]["decoupled_weight_decay"] is True
    for e in (b, sgd, w):
        e.close()


# ------------------------------------------------------------------ rejections, defaults
def test_op_rejects_bad_adam_arguments():
    eng = _engine(torch.bfloat16, 32)
    name, base = eng.update_launch("step", B=8, grid=8, exchange=False)
    assert name == "lenet_update_adam"
    good = torch.zeros(NP + 4, device=DEV)
    bad = [("mom, dampening and nesterov", base._replace(mom=0.5)),
           ("16-byte aligned", base._replace(adam_v=good[1:NP + 1])),
           ("one value per parameter", base._replace(adam_v=good[:NP - 4])),
           ("float32", base._replace(adam_v=good[:NP].double())),
           ("parameters' device", base._replace(adam_v=torch.zeros(NP))),
           (r"beta2 must be in \[0, 1\)", base._replace(beta2=1.0)),
           (r"beta1 must be in \[0, 1\)", base._replace(beta1=-0.1)),
           ("eps must be positive", base._replace(eps=0.0))]
    p0 = eng.flat.data.clone()
    for msg, args in bad:
        with pytest.raises(RuntimeError, match=msg):
            torch.ops.csed.lenet_update_adam(*args)
    st = torch.classes.csed.LenetStepper()
    with pytest.raises(RuntimeError, match="eps must be positive"):
        st.set_update_adam(*base._replace(cursor=eng.cursor, eps=0.0))
    torch.cuda.synchronize()
    assert torch.equal(eng.flat.data, p0), "a rejected call launched something"


def test_default_engine_issues_only_sgd_launches():
    from csed_514_project_distributed_training_using_pytorch_amd.engine import fused
    from csed_514_project_distributed_training_using_pytorch_amd.engine.replay import launch_key

    eng = _trainer(optimizer="sgd", momentum=0.5)
    assert eng.adam_v is None and not eng.adam
    eng.set_epoch_order(torch.arange(68) % 64)  # (8 full steps and a tail of 4)
    launches = eng._step_launches() + eng._tail_launches()[:2]
    assert [n for n, _ in launches] == ["lenet_train", "lenet_update"] * 2
    upd = launches[1][1]
    assert type(upd) is fused.UpdateArgs and len(upd) == len(fused.UPDATE_FIELDS) and upd.mom == 0.5
    key = launch_key([("lenet_train", tuple(eng.train_args(stage_next=True))), ("lenet_update", tuple(eng.update_args("step")))])
    assert launch_key(eng._step_launches()) == key, "the default engine's launch key changed"
    adam = _trainer()
    k1 = launch_key(adam._step_launches())
    adam.eps = 1e-6
    k2 = launch_key(adam._step_launches())
    adam.betas = (0.8, 0.999)
    assert len({k1, k2, launch_key(adam._step_launches())}) == 3, "a changed beta or eps needs its own capture"
    eng.close(), adam.close()


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))  # (the package, as pytest finds it)
    assert sys.argv[1:] == ["split-k"] and os.environ.get("CSED_FC_SLICES") == "2"
    run_split_k_case()
    print("split-k ok")
