"""The fused engine's argument lists (engine/fused.py TRAIN_FIELDS / UPDATE_FIELDS, filled in by
FusedLeNetTrainer.train_args / update_args) against the extension's own schemas: a schema change in
csrc/bindings.cpp that is not followed there fails here, without a GPU."""
import pytest
import torch

from csed_514_project_distributed_training_using_pytorch_amd.engine import fused
from csed_514_project_distributed_training_using_pytorch_amd.ops import _native


@pytest.fixture(scope="module")
def schemas():
    if not _native.load(build_if_missing=False):
        pytest.skip("native extension not built")
    ops = torch.ops.csed
    return {"train": ops.lenet_train.default._schema.arguments, "update": ops.lenet_update.default._schema.arguments}


def test_field_lists_are_the_op_schemas(schemas):
    assert tuple(a.name for a in schemas["train"]) == fused.TRAIN_FIELDS == fused.TrainArgs._fields
    assert tuple(a.name for a in schemas["update"]) == fused.UPDATE_FIELDS == fused.UpdateArgs._fields


def test_layout_names_every_value(schemas):
    assert len(fused.LenetLayout._fields) == len(torch.ops.csed.lenet_layout())
    assert tuple(fused.lenet_layout()) == tuple(int(v) for v in torch.ops.csed.lenet_layout())


def test_plan_and_geometry_name_every_value(schemas):
    """LenetPlan / LenetGeometry: one field per value of csed::lenet_plan (its integers, then the message) and
    csed::lenet_geometry, and the wrappers return exactly those values.  No GPU: integer arguments only."""
    ops = torch.ops.csed
    values, error = ops.lenet_plan(1024, 256, 1, 0, True, True, True, True)
    assert len(fused.LenetPlan._fields) == len(values) + 1
    assert tuple(fused.lenet_plan(1024, 256, 1, 0, True, True, True, True)) == (*(int(v) for v in values), error) \
        == (fused.TILE, fused.STRIDED, 256, 1, 1024, "")
    assert "256 workgroups" in fused.lenet_plan(65, 260, 1, 0, True).error
    geo = ops.lenet_geometry(8, 1, 0, True)
    assert len(fused.LenetGeometry._fields) == len(geo)
    assert tuple(fused.lenet_geometry(8, 1)) == tuple(int(v) for v in geo) == (32, 1, 1, 0, 32)
    lay = fused.lenet_layout()
    assert lay.vec_len == 464 and lay.fc_part_elems == 8 * 88 * 256 + 88
    assert (lay.fc_tiles, lay.conv_blocks, lay.fc_counters_off, lay.fc_part_min_batch) == (88, 84, 8 * 88 * 256, 1025)
    assert [fused.tile_grid(B) for B in (1, 4, 5, 1023, 1024, 8192)] == [1, 1, 2, 256, 256, 256]


def test_update_plan_names_every_value(schemas):
    """LenetUpdatePlan: one field per value of csed::lenet_update_plan (its integers, then the message), the
    wrapper returns exactly those values, and a bad combination carries the plan's sentence -- the one
    csed::lenet_update raises.  No GPU: integer arguments only."""
    lay = fused.lenet_layout()
    raw = (2051, True, False, True, 0, False, 0, True, False, False, True, 0, lay.fc_part_elems, 0)
    values, error = torch.ops.csed.lenet_update_plan(*raw)
    assert len(fused.LenetUpdatePlan._fields) == len(values) + 1
    plan = fused.lenet_update_plan(2051, fc_part_n=lay.fc_part_elems, forced_slices=0)
    assert tuple(plan) == (*(int(v) for v in values), error) \
        == (fused.UPDATE_SPLIT_K, 0, 0, 0, 260, 176, 8, 1, 2, 1, 2, "")
    assert tuple(fused.lenet_update_plan(257, forced_slices=0)) == (fused.UPDATE_PLAIN, 0, 0, 0, 44 + 84, 44, 4, 2, 1, 0, 1, "")
    loop = fused.lenet_update_plan(8, exch_world=2, exch_loopback=True, lr_table=True)
    assert (loop.form, loop.world_bound, loop.loopback, loop.sched, loop.blocks) == (fused.UPDATE_EXCHANGE, 2, 1, 1, 172)
    assert fused.lenet_update_plan(8, apply_sgd=True, grad_in=True).form == fused.UPDATE_SGD
    assert "reduce-only mode applies no SGD step and takes no lr_table" in \
        fused.lenet_update_plan(8, apply_sgd=False, lr_table=True).error
    assert "the fused exchange reduces the slabs itself (no grad_in)" in \
        fused.lenet_update_plan(8, grad_in=True, exch_world=2).error
    assert "words per sender" in fused.lenet_update_plan(8, exch_world=2, exch_cap=lay.exch_words - 1).error


@pytest.mark.parametrize("shape", [(1, 5, 5, 10), (10, 5, 5, 20)])
def test_wgrad_workspace_is_the_extensions(schemas, shape):
    """ops/functional.py wgrad_workspace_elems is csed::conv2d_wgrad_workspace, for the two LeNet convs
    (IC, KH, KW, OC): one [OC, IC * KH * KW + 1] slab per block, never more than 256 blocks."""
    from csed_514_project_distributed_training_using_pytorch_amd.ops.functional import wgrad_workspace_elems

    IC, KH, KW, OC = shape
    slab = OC * (IC * KH * KW + 1)
    for N in (1, 255, 256, 257, 2047, 2048, 5000):
        n = wgrad_workspace_elems(N, IC, KH, KW, OC)
        assert n == torch.ops.csed.conv2d_wgrad_workspace(N, IC, KH, KW, OC)
        assert n % slab == 0 and 1 <= n // slab <= min(N, 256)


@pytest.mark.parametrize("method,op", [("set_train", "train"), ("set_update", "update")])
def test_stepper_takes_the_op_argument_lists(schemas, method, op):
    """LenetStepper.set_train / set_update: the ops' argument types, in order (after the object itself)."""
    args = torch.classes.csed.LenetStepper()._get_method(method).schema.arguments[1:]
    assert [str(a.type) for a in args] == [str(a.type) for a in schemas[op]]
