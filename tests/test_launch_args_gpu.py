"""FusedLeNetTrainer.train_args / update_args on a real engine: global batch 8 on 64 synthetic images,
the smallest staged split-step shape (4 workgroups per sample), where the staging and grid derivation
of the builders can go wrong."""
import pytest
import torch

from csed_514_project_distributed_training_using_pytorch_amd.data import synthetic_mnist
from csed_514_project_distributed_training_using_pytorch_amd.engine.fused import FusedLeNetTrainer
from csed_514_project_distributed_training_using_pytorch_amd.models import Net

pytestmark = pytest.mark.gpu


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

    # one eager step and one native-executor step from the same state: bitwise the same state after
    eng.set_epoch_order(torch.arange(64))
    state = eng._state()
    start = [t.clone() for t in state]
    eng.step()
    eager = [t.clone() for t in state]
    for t, v in zip(state, start):
        t.copy_(v)
    eng.stepper().run(1)
    torch.cuda.synchronize()
    assert eng.cursor.item() == 1 and not torch.equal(eng.flat.data, start[0])
    for name, a, b in zip(("params", "momentum", "wimg", "step", "cursor", "rng", "loss", "xstage", "lstage"),
                          eager, state):
        assert torch.equal(a, b), name
    eng.close()
