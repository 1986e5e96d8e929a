"""Device-resident learning-rate schedules on the GPU (optim/schedule.py; csed::sgd_flat / csed::lenet_update
with lr_table / lr_pos).  The oracle everywhere is the existing constant-lr path driven step by step from the
host with the table's own fp32 values: the scheduled kernel performs the same fmaf(-lr, d, p) with a
bit-identical lr, so every comparison is torch.equal.  The tables change every step and are shorter than the
runs (5 entries for 7 steps), so the clamp to the last entry is exercised too."""
import pytest
import torch

from csed_514_project_distributed_training_using_pytorch_amd.data import synthetic_mnist
from csed_514_project_distributed_training_using_pytorch_amd.engine.fused import FusedLeNetTrainer, lenet_layout
from csed_514_project_distributed_training_using_pytorch_amd.models import Net
from csed_514_project_distributed_training_using_pytorch_amd.optim import LRSchedule

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
TABLE = [0.05, 0.08, 0.1, 0.06, 0.02]
STEPS = 7
NAMES = ("params", "momentum", "wimg", "step", "cursor", "rng", "loss", "xstage", "lstage")


def _host_lr(table: torch.Tensor, t: int) -> float:
    return float(table[min(t, table.numel() - 1)])


@pytest.mark.parametrize("n", [21840, 1027, 3])
def test_sgd_flat_schedule_is_the_host_driven_launches(n):
    """22 blocks / a scalar tail / fewer elements than one float4."""
    ops = torch.ops.csed
    gen = torch.Generator().manual_seed(n)
    p0 = torch.randn(n, generator=gen)
    grads = [torch.randn(n, generator=gen).to(DEV) for _ in range(STEPS)]
    sch = LRSchedule(torch.tensor(TABLE)).to(DEV)
    out = []
    for scheduled in (False, True):
        p, buf = p0.to(DEV), torch.zeros(n, device=DEV)
        step, ticket = torch.zeros(1, dtype=torch.long, device=DEV), torch.zeros(1, dtype=torch.int32, device=DEV)
        for t in range(STEPS):
            lr = 123.0 if scheduled else _host_lr(sch.table.cpu(), t)  # (a scheduled launch ignores the scalar)
            extra = (sch.table, sch.pos) if scheduled else ()
            ops.sgd_flat(p, grads[t], buf, lr, 0.5, 0.0, 0.01, True, 1.0, step, ticket, *extra)
        torch.cuda.synchronize()
        assert ticket.item() == 0 and step.item() == STEPS
        out.append((p, buf))
    assert sch.position() == STEPS
    assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1], out[1][1])
    assert torch.isfinite(out[1][0]).all() and not torch.equal(out[1][0], p0.to(DEV))


def _restore(eng, state, start):
    torch.cuda.synchronize()
    for t, v in zip(state, start):
        t.copy_(v)


@pytest.mark.parametrize("dtype,dampening", [(torch.bfloat16, 0.0), (torch.float32, 0.0), (torch.bfloat16, 0.1)])
def test_fused_engine_eager_graphs_and_stepper(dtype, dampening):
    """Global batch 8 on 64 synthetic images (grid 32, the staged split step): 7 scheduled steps eagerly,
    through one graph and through the native executor, against 7 eager steps whose lr the host sets.  With
    dampening the kernel's first-step flag and the schedule share the ticket."""
    torch.manual_seed(1)
    eng = FusedLeNetTrainer(Net().to(DEV), synthetic_mnist(64, seed=3), momentum=0.5, dampening=dampening,
                            global_batch=8, compute_dtype=dtype)
    assert eng.staged and eng.split and eng.grid == 32
    eng.set_epoch_order(torch.arange(64))
    table = torch.tensor(TABLE)
    start = [t.clone() for t in eng._state()]
    for t in range(STEPS):
        eng.lr = _host_lr(table, t)
        eng.step()
    torch.cuda.synchronize()
    ref = [t.clone() for t in eng._state()]
    assert not torch.equal(ref[0], start[0]) and torch.isfinite(ref[0]).all()

    eng.lr = 123.0  # (never used once a schedule is set)
    sch = LRSchedule(table)
    eng.set_lr_schedule(sch)
    assert eng._state()[-1] is sch.pos and sch.device == eng.device
    runs = {"eager": lambda: [eng.step() for _ in range(STEPS)],
            "graphs": lambda: eng.run_steps(STEPS),
            "stepper": lambda: eng.stepper().run(STEPS)}
    for name, run in runs.items():
        _restore(eng, eng._state()[:-1], start)
        sch.set_position(0)
        assert eng.optimizer_state_dict()["param_groups"][0]["lr"] == table[0].item()
        run()
        torch.cuda.synchronize()
        assert sch.position() == STEPS and eng.ticket.item() == 0, name
        for what, a, b in zip(NAMES, ref, eng._state()):
            assert torch.equal(a, b), (name, what)
    assert len(eng._graphs) == 1
    assert eng.optimizer_state_dict()["param_groups"][0]["lr"] == table[-1].item()
    eng.close()


def test_reduce_then_apply_by_hand():
    """Mode "apply" (lenet_sgd_kernel) reads and advances the schedule, mode "reduce" does neither."""
    ops = torch.ops.csed
    torch.manual_seed(1)
    eng = FusedLeNetTrainer(Net().to(DEV), synthetic_mnist(64, seed=3), momentum=0.5, global_batch=8)
    eng.set_epoch_order(torch.arange(64))
    table = torch.tensor(TABLE)
    g = torch.empty(21840, device=DEV)
    start = [t.clone() for t in eng._state()]

    def pairs():
        for t in range(STEPS):
            if eng.lr_schedule is None:
                eng.lr = _host_lr(table, t)
            ops.lenet_train(*eng.train_args())
            ops.lenet_update(*eng.update_args("reduce", grad=g))
            if eng.lr_schedule is not None:
                assert eng.lr_schedule.position() == t  # ("reduce" alone leaves it unchanged)
            ops.lenet_update(*eng.update_args("apply", grad=g))
            if eng.lr_schedule is not None:
                assert eng.lr_schedule.position() == t + 1  # (once per pair)
        torch.cuda.synchronize()

    pairs()
    ref = [t.clone() for t in eng._state()]
    sch = LRSchedule(table)
    eng.set_lr_schedule(sch)
    _restore(eng, eng._state()[:-1], start)
    pairs()
    assert eng.ticket.item() == 0 and eng.step_count.item() == ref[3].item()
    for what, a, b in zip(NAMES, ref, eng._state()):
        assert torch.equal(a, b), what
    bad = eng.update_args("reduce", grad=g)._replace(lr_table=sch.table, lr_pos=sch.pos)
    assert bad.apply_sgd is False
    with pytest.raises(RuntimeError, match="reduce-only"):
        ops.lenet_update(*bad)
    with pytest.raises(RuntimeError, match="float32"):
        ops.lenet_update(*eng.update_args("step")._replace(lr_table=sch.table.double()))
    with pytest.raises(RuntimeError, match="GPU tensor"):
        ops.lenet_update(*eng.update_args("step")._replace(lr_table=sch.table.cpu()))
    torch.cuda.synchronize()
    assert sch.position() == STEPS
    eng.close()


def test_exchange_variant_loopback_is_local_training():
    """The XW > 0 instantiations (loopback world 2, with its invariant check): as in
    test_exchange_loopback_gpu, the looped-back training is bitwise the world-1 training -- here both on
    the same schedule, through graphs and the native executor."""
    finals = []
    for world in (0, 2):
        torch.manual_seed(1)
        eng = FusedLeNetTrainer(Net().to(DEV), synthetic_mnist(2048, seed=3), lr=0.05, momentum=0.5, global_batch=16,
                                loopback_world=world)
        sch = LRSchedule(torch.tensor(TABLE))
        eng.set_lr_schedule(sch)
        eng.set_epoch_order(torch.randperm(2048, generator=torch.Generator().manual_seed(0)))
        eng.run_steps(8, steps_per_graph=4)
        eng.run_steps(4, use_graph=False)
        torch.cuda.synchronize()
        assert eng.comm_errors() == 0 and sch.position() == 12 and eng.ticket.item() == 0
        assert eng.allreduce_kind == ("none" if world == 0 else "fused-ipc-loopback2")
        finals.append(eng.flat.data.clone())
        eng.close()
    assert torch.isfinite(finals[0]).all()
    assert torch.equal(finals[0], finals[1])


@pytest.mark.parametrize("shape", ["tile_min_batch", "split_k"])
def test_tile_kernel_and_split_k_fc_update(shape):
    """Per-rank batch tile_min_batch (the sample-tile kernel) and 2048 (also the split-K fc update, whose
    last-arriving slice finishes a tile): 3 scheduled graph-replayed steps against host-driven constant lr."""
    steps, B = 3, lenet_layout().tile_min_batch if shape == "tile_min_batch" else 2048
    data = synthetic_mnist(steps * B, seed=6)
    table = torch.tensor(TABLE[:2])  # (shorter than the run: the third step clamps)
    out = []
    for scheduled in (False, True):
        torch.manual_seed(4)
        eng = FusedLeNetTrainer(Net().to(DEV), data, lr=0.05, momentum=0.9, global_batch=B,
                                compute_dtype=torch.float16)
        assert eng.uses_tile_kernel() and (eng.fc_part is not None) == (B > 1024)
        eng.set_epoch_order(torch.arange(steps * B))
        if scheduled:
            sch = LRSchedule(table)
            eng.set_lr_schedule(sch)
            eng.run_steps(steps)
        else:
            for t in range(steps):
                eng.lr = _host_lr(table, t)
                eng.step()
        torch.cuda.synchronize()
        assert eng.ticket.item() == 0
        if eng.fc_part is not None:  # every tile's arrival counter back at zero, as after an unscheduled step
            assert eng.fc_counters().numel() == 88 and int(eng.fc_counters().abs().sum().item()) == 0
        if scheduled:
            assert sch.position() == steps
        out.append([t.clone() for t in eng._state()[:7]])
        eng.close()
    assert torch.isfinite(out[0][0]).all()
    for what, a, b in zip(NAMES, out[0], out[1]):
        assert torch.equal(a, b), what


def _modular_batches(n, B):
    g = torch.Generator(device=DEV).manual_seed(7)
    return [(torch.randn(B, 1, 28, 28, device=DEV, generator=g).to(torch.bfloat16),
             torch.randint(0, 10, (B,), device=DEV, generator=g)) for _ in range(n)]


def test_modular_engine_one_capture_serves_the_schedule():
    from csed_514_project_distributed_training_using_pytorch_amd.engine.modular import ModularTrainer

    batches = _modular_batches(6, 16)
    table = torch.tensor(TABLE)
    res = {}
    for kind in ("graph", "eager", "host"):
        torch.manual_seed(1)
        tr = ModularTrainer(Net().cuda().train(), lr=0.05, momentum=0.5, graph=kind == "graph")
        if kind != "host":
            tr.opt.set_lr_schedule(LRSchedule(table))
        for i, (x, t) in enumerate(batches):
            if kind == "host":
                tr.opt.param_groups[0]["lr"] = _host_lr(table, i)
            tr.train_batch(x, t)
        torch.cuda.synchronize()
        res[kind] = tr
    assert res["graph"].use_graph and len(res["graph"]._graphs) == 1
    for kind in ("graph", "eager"):
        assert res[kind].opt.lr_schedule.position() == 6 and res[kind].opt._ticket.item() == 0
        assert res[kind].opt.state_dict()["param_groups"][0]["lr"] == table[-1].item()
    for other in ("eager", "host"):
        assert torch.equal(res["graph"].flat.data, res[other].flat.data), other
        assert torch.equal(res["graph"].opt.momentum_flat, res[other].opt.momentum_flat), other
    assert torch.isfinite(res["graph"].flat.data).all()


def test_set_lr_schedule_drops_graphs_and_stepper():
    """Resume on the device: a new schedule (a checkpoint's table and position) set after graphs and the
    executor exist -- the following replay trains at the new table's values from its position."""
    torch.manual_seed(1)
    eng = FusedLeNetTrainer(Net().to(DEV), synthetic_mnist(64, seed=3), momentum=0.5, global_batch=8)
    eng.set_epoch_order(torch.arange(64))
    eng.set_lr_schedule(LRSchedule(torch.tensor(TABLE)))
    eng.run_steps(2)
    eng.stepper().run(1)
    torch.cuda.synchronize()
    assert eng._graphs and eng._stepper is not None
    mid = [t.clone() for t in eng._state()[:-1]]
    new = torch.tensor([0.5, 0.4, 0.03, 0.07, 0.011, 0.09])
    resumed = LRSchedule.from_state_dict({"table": new, "t": 2})
    eng.set_lr_schedule(resumed)
    assert not eng._graphs and eng._stepper is None
    eng.run_steps(3)
    eng.stepper().run(2)
    torch.cuda.synchronize()
    got = [t.clone() for t in eng._state()[:-1]]
    assert resumed.position() == 7
    eng.set_lr_schedule(None)
    _restore(eng, eng._state(), mid)
    for t in range(2, 7):
        eng.lr = _host_lr(new, t)
        eng.step()
    torch.cuda.synchronize()
    for what, a, b in zip(NAMES, got, eng._state()):
        assert torch.equal(a, b), what
    eng.close()
