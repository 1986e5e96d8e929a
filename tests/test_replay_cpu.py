"""engine/replay.py without a GPU: launch_key over real TrainArgs / UpdateArgs tuples filled with CPU tensors
(what the fused engine's graph cache and native executor are keyed on), graph_plan and preserved."""
import pytest
import torch

from csed_514_project_distributed_training_using_pytorch_amd.engine import fused
from csed_514_project_distributed_training_using_pytorch_amd.engine.replay import graph_plan, launch_key, preserved

FusedLeNetTrainer, TrainArgs, UpdateArgs = fused.FusedLeNetTrainer, fused.TrainArgs, fused.UpdateArgs


def _buffers() -> dict:
    f, i = torch.float32, torch.long
    return dict(images=torch.zeros(40, 784, dtype=torch.uint8), labels=torch.zeros(40, dtype=i), perm=torch.arange(40),
                cursor=torch.zeros(1, dtype=i), wimg=torch.zeros(64, dtype=torch.int16), params=torch.zeros(32),
                slab=torch.zeros(16, 8, dtype=f), vslab=torch.zeros(64, 4, dtype=f), loss_parts=torch.zeros(32),
                rng_offset=torch.zeros(1, dtype=i), xstage=torch.zeros(16, 784, dtype=torch.uint8),
                lstage=torch.zeros(16, dtype=i), momentum=torch.zeros(32, dtype=f), step=torch.zeros(1, dtype=i),
                ticket=torch.zeros(1, dtype=torch.int32), loss_acc=torch.zeros(2, dtype=f))


def _step(b: dict, perm=None, lr=0.01, kernel=0, staged=True) -> list:
    """One step's launches, as FusedLeNetTrainer._step_launches lists them."""
    train = TrainArgs(
        images=b["images"], labels=b["labels"], perm=b["perm"] if perm is None else perm, cursor=b["cursor"], B=16,
        rank=0, wimg=b["wimg"], params=b["params"], slab=b["slab"], vslab=b["vslab"], loss_parts=b["loss_parts"],
        grad_scale=1.0, mean=0.1307, std=0.3081, drop_p=0.5, seed=1, rng_offset=b["rng_offset"], grid=16, mfma_dtype=1,
        dbg=None, xstage=b["xstage"] if staged else None, lstage=b["lstage"] if staged else None, stage_next=staged,
        kernel=kernel)
    update = UpdateArgs(
        slab=b["slab"], grid=16, vslab=b["vslab"], B=16, grad_in=None, grad_out=None, params=b["params"],
        momentum=b["momentum"], wimg=b["wimg"], lr=lr, mom=0.5, dampening=0.0, weight_decay=0.0, nesterov=False,
        step=b["step"], ticket=b["ticket"], cursor=b["cursor"], rng_offset=b["rng_offset"], apply_sgd=True,
        loss_parts=b["loss_parts"], nparts=16, loss_acc=b["loss_acc"], mfma_dtype=1, dbg=None, exch_id=-1,
        exch_timeout_s=2.0, grad_post=1.0 / 16, fc_part=None, lr_table=None, lr_pos=None)
    return [("lenet_train", train), ("lenet_update", update)]


def test_launch_key_is_what_the_launches_point_at_and_hold():
    b = _buffers()
    key = launch_key(_step(b))
    assert key == launch_key(_step(b)) and hash(key) == hash(launch_key(_step(b)))  # the same tuples built twice
    assert key[0][0] == "lenet_train" and len(key[0][1]) == len(TrainArgs._fields)
    assert key[1][1][UpdateArgs._fields.index("params")] == (b["params"].data_ptr(), 32, torch.float32)
    other = dict(b, params=torch.zeros(32))  # another storage of the same shape
    assert launch_key(_step(other)) != key
    # a view at another offset: the epoch's tail against its head
    assert launch_key(_step(b, perm=b["perm"][8:])) != launch_key(_step(b, perm=b["perm"][:8]))
    assert launch_key(_step(b, perm=b["perm"][:32])) != key  # the same address, fewer elements
    assert launch_key(_step(b, staged=False)) != key  # None in a tensor's place
    assert launch_key(_step(b, lr=0.02)) != key  # one float field
    assert launch_key(_step(b, kernel=1)) != key  # one int field
    assert launch_key(_step(b)[:1]) != key and launch_key(None) is None and launch_key(3) == 3


@pytest.mark.parametrize("k,spg,sizes", [(0, 16, []), (20, 16, [16, 4]), (5, 16, [5]), (32, 16, [16, 16]),
                                         (3, 1, [1, 1, 1])])
def test_graph_plan(k, spg, sizes):
    assert graph_plan(k, spg) == sizes == FusedLeNetTrainer.graph_plan(k, spg)


def test_preserved_restores_after_exit_and_after_an_exception():
    a, b = torch.arange(4.0), torch.ones(3, dtype=torch.long)
    with preserved([a, b]):
        a.add_(1)
        b.zero_()
        assert a[0] == 1 and b.sum() == 0
    assert torch.equal(a, torch.arange(4.0)) and torch.equal(b, torch.ones(3, dtype=torch.long))
    with pytest.raises(KeyError):
        with preserved([a, b]):
            a.mul_(3)
            b.fill_(7)
            raise KeyError("step failed")
    assert torch.equal(a, torch.arange(4.0)) and torch.equal(b, torch.ones(3, dtype=torch.long))
