"""FusedLeNetTrainer.train_args / update_args on real engines: global batch 8 on 64 synthetic images, the
smallest staged split-step shape (4 workgroups per sample), where the staging and grid derivation of the
builders can go wrong; the engine's geometry on either side of every threshold of the launch plan
(csrc/kernels/lenet_plan.h); and the launches the plan rejects."""
import pytest
import torch

from csed_514_project_distributed_training_using_pytorch_amd.data import synthetic_mnist
from csed_514_project_distributed_training_using_pytorch_amd.engine.fused import (
    UPDATE_EXCHANGE, UPDATE_PLAIN, UPDATE_SPLIT_K, FusedLeNetTrainer, lenet_layout)
from csed_514_project_distributed_training_using_pytorch_amd.models import Net

pytestmark = pytest.mark.gpu

STATE = ("params", "momentum", "wimg", "step", "cursor", "rng", "loss", "xstage", "lstage")


def _eager_and_stepper_agree(eng, n):
    """One eager step and one native-executor step from the same state: bitwise the same state after."""
    eng.set_epoch_order(torch.arange(n))
    state = eng._state()
    start = [t.clone() for t in state]
    eng.step()
    eager = [t.clone() for t in state]
    for t, v in zip(state, start):
        t.copy_(v)
    eng.stepper().run(1)
    torch.cuda.synchronize()
    assert eng.cursor.item() == 1 and not torch.equal(eng.flat.data, start[0])
    for name, a, b in zip(STATE, eager, state):
        assert torch.equal(a, b), name


def test_builder_modes_and_stepper_matches_eager_step():
    dev = torch.device("cuda", 0)
    torch.manual_seed(1)
    eng = FusedLeNetTrainer(Net().to(dev), synthetic_mnist(64, seed=3), global_batch=8)
    assert eng.staged and eng.split and eng.grid == 32
    ops = torch.ops.csed
    train, step = eng.train_args(), eng.update_args("step")
    assert len(train) == len(ops.lenet_train.default._schema.arguments)
    assert len(step) == len(ops.lenet_update.default._schema.arguments)
    assert train.xstage is eng.xstage and train.grid == step.grid == 32 and step.cursor is eng.cursor

    g = torch.empty(21840, device=dev)
    reduce = eng.update_args("reduce", grad=g)
    assert reduce.cursor is None and reduce.apply_sgd is False and reduce.grad_out is g and reduce.grad_in is None
    apply = eng.update_args("apply", grad=g)
    assert apply.grad_in is g and apply.grad_out is None and apply.apply_sgd is True
    assert apply.loss_parts is None and apply.loss_acc is None and apply.nparts == 0

    _eager_and_stepper_agree(eng, 64)
    eng.close()


# (dtype, per-rank batch) -> grid, split, staged, tile_staged, staging rows, tile kernel, training kernel: the
# engine's defaults on either side of each threshold (split step up to 64, staging up to 256, tile kernel from 1024;
# fp32 stages only in the split step)
BOUNDARIES = {
    (torch.bfloat16, 8): (32, True, True, False, 32, False, "lenet_train"),
    (torch.bfloat16, 64): (256, True, True, False, 256, False, "lenet_train"),
    (torch.bfloat16, 65): (65, False, True, False, 65, False, "lenet_train"),
    (torch.bfloat16, 256): (256, False, True, False, 256, False, "lenet_train"),
    (torch.bfloat16, 257): (256, False, False, False, 0, False, "lenet_train"),
    (torch.bfloat16, 1023): (256, False, False, False, 0, False, "lenet_train"),
    (torch.bfloat16, 1024): (256, False, False, True, 1024, True, "lenet_tile"),
    (torch.float32, 64): (256, True, True, False, 256, False, "lenet_train_f32"),
    (torch.float32, 65): (65, False, False, False, 0, False, "lenet_train_f32"),
}


@pytest.mark.parametrize("dtype,B", list(BOUNDARIES), ids=lambda v: str(v).replace("torch.", ""))
def test_engine_geometry_at_the_plan_boundaries(dtype, B):
    grid, split, staged, tile_staged, rows, tile, kernel = BOUNDARIES[dtype, B]
    torch.manual_seed(1)
    eng = FusedLeNetTrainer(Net().to("cuda:0"), synthetic_mnist(2 * B, seed=3), global_batch=B, compute_dtype=dtype)
    assert (eng.grid, eng.split, eng.staged, eng.tile_staged) == (grid, split, staged, tile_staged)
    assert (0 if eng.xstage is None else eng.xstage.shape[0]) == rows
    assert (0 if eng.lstage is None else eng.lstage.shape[0]) == rows
    assert eng.uses_tile_kernel() is tile and eng.kernel_names == kernel + " + lenet_update"
    assert (eng.train_args().xstage is not None) == (rows > 0)
    _eager_and_stepper_agree(eng, 2 * B)
    eng.close()


def _bare_engine(B, grid, **kw):
    """An engine whose training kernels never run (zero images): lenet_update alone, on filled slabs."""
    from csed_514_project_distributed_training_using_pytorch_amd.data.mnist import MNISTData

    data = MNISTData(torch.zeros((B, 28, 28), dtype=torch.uint8), torch.zeros(B, dtype=torch.long), True)
    torch.manual_seed(1)
    return FusedLeNetTrainer(Net().to("cuda:0"), data, global_batch=B, grid=grid, **kw)


def _stamped_update(eng, B, grid):
    """One "step" update at per-rank batch B on integer slabs (csed::lenet_selftest_fill) with the block stamps
    on, checked against its plan.  Every block stamps slot 0 at the top of update_role, so the stamped rows are
    the blocks that ran.  The stamps carry no role, so the FC / CONV boundary is checked through the work: from a
    zero momentum buffer the step leaves the gradient there, and a grid whose first plan.fc_blocks blocks were not
    exactly the FC role would leave FC tiles or conv slab chunks (whole runs of parameters) unfinished."""
    ops = torch.ops.csed
    args = eng.update_args("step", B=B, grid=grid, dbg=torch.zeros(1024, 8, dtype=torch.long, device=eng.device))
    plan = eng.update_plan(args)
    assert not plan.error
    ops.lenet_selftest_fill(eng.slab, eng.vslab, B, eng.mfma, 977 + B)
    eng.momentum_buf.zero_()
    ops.lenet_update(*args)
    torch.cuda.synchronize()
    ran = (args.dbg[:, 0] != 0).cpu()
    assert int(ran.sum()) == plan.blocks and bool(ran[:plan.blocks].all())
    assert bool((args.dbg[:plan.blocks, 4] != 0).all())  # each of them got to its end
    lay = lenet_layout()
    assert plan.blocks - plan.fc_blocks == lay.conv_blocks
    assert plan.fc_blocks == plan.slices * -(-lay.fc_tiles // plan.tiles_per_block)
    assert torch.isfinite(eng.momentum_buf).all()
    assert bool((eng.momentum_buf.view(-1, 16) != 0).any(dim=1).all()), "a run of 16 parameters got no gradient"
    return plan


def test_update_launcher_follows_its_plan():
    """The grid csed::lenet_update launches is csed::lenet_update_plan's (csrc/kernels/lenet_plan.h), at one
    batch per waves-per-tile class, at two split-K slices and through a loopback exchange of world 2."""
    eng = _bare_engine(513, 64)
    assert eng.fc_part is None
    want = {8: (1, 1, 88), 33: (1, 1, 88), 129: (2, 4, 22), 257: (4, 2, 44), 513: (8, 1, 88)}
    for B, (wpt, tpb, nfc) in want.items():
        plan = _stamped_update(eng, B, min(B, 64))
        assert (plan.form, plan.waves_per_tile, plan.tiles_per_block, plan.fc_blocks, plan.blocks) == \
            (UPDATE_PLAIN, wpt, tpb, nfc, nfc + 84), B
    eng.close()

    eng = _bare_engine(2051, 64)
    assert eng.fc_part is not None
    plan = _stamped_update(eng, 2051, 64)
    assert (plan.form, plan.slices, plan.fc_blocks, plan.blocks) == (UPDATE_SPLIT_K, 2, 176, 260)
    assert int(eng.fc_counters().abs().sum().item()) == 0
    eng.close()

    eng = _bare_engine(8, 8, loopback_world=2)
    plan = _stamped_update(eng, 8, 8)
    assert (plan.form, plan.world_bound, plan.loopback, plan.fc_blocks, plan.blocks) == (UPDATE_EXCHANGE, 2, 1, 88, 172)
    assert eng.comm_errors() == 0
    g = torch.zeros(21840, device=eng.device)
    with pytest.raises(RuntimeError, match="lenet_update: the fused exchange reduces the slabs itself"):
        torch.ops.csed.lenet_update(*eng.update_args("step")._replace(grad_in=g))
    # the native executor resolves the plan when it takes the argument block, not at run()
    with pytest.raises(RuntimeError, match="lenet_update: the exchange timeout must be positive"):
        torch.classes.csed.LenetStepper().set_update(*eng.update_args("step")._replace(exch_timeout_s=0.0))
    eng.close()


def test_rejected_launches_raise_before_anything_is_enqueued():
    """Launches the plan calls invalid raise from the op's argument checks, each naming the rule; nothing
    reaches the device, so the engine trains on afterwards."""
    dev = torch.device("cuda", 0)
    torch.manual_seed(1)
    data = synthetic_mnist(64, seed=3)
    eng = FusedLeNetTrainer(Net().to(dev), data, global_batch=8)  # staged split step: B 8, grid 32
    f32 = FusedLeNetTrainer(Net().to(dev), data, global_batch=8, compute_dtype=torch.float32, split=False)
    assert not f32.staged and f32.grid == 8
    eng.set_epoch_order(torch.arange(64))
    staged, unstaged = eng.train_args(stage_next=True), dict(xstage=None, lstage=None, stage_next=False)
    xs, ls = torch.zeros(8, 784, dtype=torch.uint8, device=dev), torch.zeros(8, dtype=torch.long, device=dev)
    cases = [
        (staged._replace(kernel=2), "sample-tile kernel runs grid"),  # kernel 2 off the tile grid
        (staged._replace(B=1024, grid=200, kernel=0, **unstaged), "sample-tile kernel runs grid"),  # auto, B 1024
        (f32.train_args()._replace(xstage=xs, lstage=ls), "fp32 stages its batch only in the split step"),
        (staged._replace(B=65, grid=260), "at most 256 workgroups"),
        (staged._replace(lstage=None), "xstage and lstage go together"),
        (staged._replace(**unstaged), "grid <= B"),
        (staged._replace(cursor=None), "stage_next needs"),
    ]
    before = eng.flat.data.clone()
    for args, message in cases:
        with pytest.raises(RuntimeError, match=message):
            torch.ops.csed.lenet_train(*args)
    torch.cuda.synchronize()
    assert torch.equal(eng.flat.data, before) and eng.cursor.item() == 0
    eng.step()
    torch.cuda.synchronize()
    assert eng.cursor.item() == 1 and not torch.equal(eng.flat.data, before)
    assert torch.isfinite(eng.flat.data).all()
    eng.close()
    f32.close()
