"""optim.FusedAdam (CPU parameters): its float32 evaluation of the Adam / AdamW rule (_cpu_step) inside the derived
bounds of the fp64 oracle (tests/_adam_oracle.py) over the hyper-parameter table, with a gradient scale and a
schedule; the state dict against torch.optim.Adam's / AdamW's; a shared FlatParams.  GPU parameters are refused
(tests/test_adam_flat_gpu.py)."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _adam_flat_cases as afc  # noqa: E402

from csed_514_project_distributed_training_using_pytorch_amd.models import Net  # noqa: E402
from csed_514_project_distributed_training_using_pytorch_amd.optim import FusedAdam, LRSchedule  # noqa: E402


def _optimizer(n, hyper, start, seed):
    decoupled, wd, betas = hyper
    p, m, v = afc.make_state(n, start, seed)
    w = torch.nn.Parameter(p.clone())
    opt = FusedAdam([w], lr=afc.LR, betas=betas, eps=afc.EPS, weight_decay=wd, decoupled=decoupled)
    opt.exp_avg_flat[:n].copy_(m)
    opt.exp_avg_sq_flat[:n].copy_(v)
    opt.step_count.fill_(start)
    return w, opt


@pytest.mark.parametrize("start", afc.STARTS, ids=lambda s: "step%d" % s)
@pytest.mark.parametrize("hyper", afc.HYPER, ids=afc.hyper_id)
def test_cpu_step_stays_inside_the_bounds(hyper, start):
    """Three steps of _cpu_step (n = 1027: FlatParams pads to 1028), each from its own previous state."""
    n = 1027
    w, opt = _optimizer(n, hyper, start, seed=3)
    for k, g in enumerate(afc.make_grads(n, 3, seed=3)):
        prev = tuple(x[:n].clone() for x in (opt.flat.data, opt.exp_avg_flat, opt.exp_avg_sq_flat))
        g = afc.settle(g, prev[0])
        w.grad = g.clone()
        opt.step()
        got = (opt.flat.data[:n], opt.exp_avg_flat[:n], opt.exp_avg_sq_flat[:n])
        afc.check_step(got, prev, g, start + k + 1, hyper, what=afc.hyper_id(hyper))
    assert int(opt.step_count.item()) == start + 3
    assert not opt.flat.data[n:].any()  # (the padding stays 0)


def test_cpu_step_grad_scale_and_schedule():
    hyper = (True, 0.01, (0.9, 0.999))
    n = 257
    w, opt = _optimizer(n, hyper, 0, seed=4)
    opt.grad_scale = 0.5
    sch = LRSchedule([1e-3, 2.5e-4, 5e-4], t=1)
    opt.set_lr_schedule(sch)
    for k, (g, lr) in enumerate(zip(afc.make_grads(n, 4, seed=4), (2.5e-4, 5e-4, 5e-4, 5e-4))):
        prev = tuple(x[:n].clone() for x in (opt.flat.data, opt.exp_avg_flat, opt.exp_avg_sq_flat))
        w.grad = g.clone()
        opt.step()
        got = (opt.flat.data[:n], opt.exp_avg_flat[:n], opt.exp_avg_sq_flat[:n])
        afc.check_step(got, prev, g, k + 1, hyper, lr=lr, gscale=0.5)
    assert sch.position() == 5


@pytest.mark.parametrize("decoupled", [False, True], ids=["adam", "adamw"])
def test_state_dict_is_torchs(decoupled):
    """Keys, dtypes and shapes of torch.optim.Adam's / AdamW's own state dict after the same steps; each loads
    into the other; the other optimizer's or SGD's state raises ValueError."""
    torch.manual_seed(2)
    net_a, net_b = Net(), Net()
    net_b.load_state_dict(net_a.state_dict())
    kw = dict(lr=1e-3, betas=(0.8, 0.99), eps=1e-7, weight_decay=0.01)
    ours = FusedAdam(net_a.parameters(), decoupled=decoupled, **kw)
    theirs = (torch.optim.AdamW if decoupled else torch.optim.Adam)(net_b.parameters(), **kw)
    assert ours.state_dict()["state"] == {} == theirs.state_dict()["state"]
    for _ in range(2):
        for pa, pb in zip(net_a.parameters(), net_b.parameters()):
            pb.grad = torch.randn_like(pb)
            pa.grad = pb.grad.clone()
        ours.step()
        theirs.step()
    a, b = ours.state_dict(), theirs.state_dict()
    assert a["param_groups"] == b["param_groups"]
    assert sorted(a["state"]) == sorted(b["state"]) == list(range(8))
    for i in range(8):
        assert sorted(a["state"][i]) == sorted(b["state"][i]) == ["exp_avg", "exp_avg_sq", "step"]
        for k in a["state"][i]:
            x, y = a["state"][i][k], b["state"][i][k]
            assert (x.dtype, x.shape, x.device) == (y.dtype, y.shape, y.device), (i, k)
        assert float(a["state"][i]["step"]) == 2.0 == float(b["state"][i]["step"])  # (values: the bounds tests)
    theirs.load_state_dict(a)
    ours.load_state_dict(theirs.state_dict())
    assert int(ours.step_count.item()) == 2
    for i in range(8):
        assert torch.equal(ours.flat.view(ours.exp_avg_sq_flat, i), a["state"][i]["exp_avg_sq"])
    other = FusedAdam(Net().parameters(), decoupled=not decoupled, **kw)
    with pytest.raises(ValueError, match="AdamW" if decoupled else "Adam's"):
        other.load_state_dict(a)
    sgd = torch.optim.SGD(Net().parameters(), lr=0.1, momentum=0.5)
    with pytest.raises(ValueError, match="not Adam's"):
        ours.load_state_dict(sgd.state_dict())
    sch = LRSchedule([1e-3, 2.5e-4], t=1)
    ours.set_lr_schedule(sch)
    assert ours.state_dict()["param_groups"][0]["lr"] == sch.current_lr() == float(torch.tensor(2.5e-4))


def test_shared_flat_params():
    """``flat=``: the optimizer works on a FlatParams it is handed (the buffers a reducer would own), and refuses
    one over other parameters; state_dict() and load_state_dict() leave no second copy of the state behind."""
    from csed_514_project_distributed_training_using_pytorch_amd.utils.flat import FlatParams

    torch.manual_seed(3)
    net = Net()
    params = list(net.parameters())
    flat = FlatParams(params)
    opt = FusedAdam(params, lr=1e-3, weight_decay=0.01, decoupled=True, flat=flat)
    assert opt.flat is flat and opt.exp_avg_flat.shape == flat.data.shape
    before = flat.data.clone()
    for p in params:
        p.grad = torch.randn_like(p)
    opt.step()
    assert flat.grads_are_views() and not torch.equal(before, flat.data)
    assert params[0].data_ptr() == flat.data.data_ptr()  # (the parameters are views of the shared buffer)
    sd = opt.state_dict()
    assert len(opt.state) == 0 and float(sd["state"][7]["step"]) == 1.0
    opt.load_state_dict(sd)
    assert len(opt.state) == 0 and int(opt.step_count.item()) == 1
    with pytest.raises(ValueError, match="same order"):
        FusedAdam(params, flat=FlatParams(list(Net().parameters())))
    with pytest.raises(ValueError, match="same order"):
        FusedAdam(params[::-1], flat=flat)
