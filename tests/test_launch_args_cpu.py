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


@pytest.mark.parametrize("method,op", [("set_train", "train"), ("set_update", "update")])
def test_stepper_takes_the_op_argument_lists(schemas, method, op):
    """LenetStepper.set_train / set_update: the ops' argument types, in order (after the object itself)."""
    args = torch.classes.csed.LenetStepper()._get_method(method).schema.arguments[1:]
    assert [str(a.type) for a in args] == [str(a.type) for a in schemas[op]]
