"""Device-resident learning-rate schedules (optim/schedule.py) without a GPU: the tables against torch's own
schedulers, the clamp past the table's end, FusedSGD's CPU step on a schedule against torch.optim.SGD with the
same scheduler, the state round trip, and the CLI's --lr-schedule / --resume checkpoint."""
import math
import os
import subprocess
import sys

import pytest
import torch
from torch.optim import lr_scheduler as ls

from csed_514_project_distributed_training_using_pytorch_amd.optim import FusedSGD, LRSchedule

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WARM, TOTAL, BASE = 3, 12, 0.1


def _cosine(opt, warm=WARM, total=TOTAL, min_lr=0.005, start=0.25):
    return ls.SequentialLR(opt, [ls.LinearLR(opt, start_factor=start, end_factor=1.0, total_iters=warm),
                                 ls.CosineAnnealingLR(opt, T_max=total - warm, eta_min=min_lr)], milestones=[warm])


def _step(opt, warm=WARM, step_size=4, gamma=0.5, start=0.25):  # (4 does not divide the 9 steps after warm-up)
    return ls.SequentialLR(opt, [ls.LinearLR(opt, start_factor=start, end_factor=1.0, total_iters=warm),
                                 ls.StepLR(opt, step_size=step_size, gamma=gamma)], milestones=[warm])


def test_tables_are_the_torch_compositions():
    cos = LRSchedule.warmup_cosine(BASE, WARM, TOTAL, min_lr=0.005, start_factor=0.25)
    ref = LRSchedule.from_torch(_cosine, BASE, TOTAL)
    assert cos.table.dtype == torch.float32 and len(cos) == TOTAL
    assert torch.equal(cos.table, ref.table)
    stp = LRSchedule.warmup_step(BASE, WARM, 4, 0.5, TOTAL, start_factor=0.25)
    assert torch.equal(stp.table, LRSchedule.from_torch(_step, BASE, TOTAL).table)
    # and they are the schedules their names say (closed forms, to double rounding of torch's chained forms)
    for t in range(TOTAL):
        if t < WARM:
            want_c = want_s = BASE * (0.25 + 0.75 * t / WARM)
        else:
            want_c = 0.005 + (BASE - 0.005) * (1 + math.cos(math.pi * (t - WARM) / (TOTAL - WARM))) / 2
            want_s = BASE * 0.5 ** ((t - WARM) // 4)
        assert cos.table[t].item() == pytest.approx(want_c, rel=1e-6), t
        assert stp.table[t].item() == pytest.approx(want_s, rel=1e-6), t
    assert torch.equal(LRSchedule.constant(0.3, 4).table, torch.full((4,), 0.3))


def test_position_clamps_to_the_last_entry():
    s = LRSchedule(torch.tensor([0.4, 0.3, 0.2]))
    assert s.current_lr() == pytest.approx(0.4)
    for t in (2, 3, 100):
        s.set_position(t)
        assert s.position() == t and s.current_lr() == s.table[2].item()
    with pytest.raises(ValueError):
        LRSchedule(torch.empty(0))


def _params(seed=0):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(7, 5, generator=g, requires_grad=True), torch.randn(11, generator=g, requires_grad=True)]


def _set_grads(params, step):
    g = torch.Generator().manual_seed(100 + step)
    for p in params:
        p.grad = torch.randn(p.shape, generator=g)


@pytest.mark.parametrize("nesterov,wd", [(False, 0.0), (True, 0.01)])
def test_cpu_optimizer_follows_the_torch_scheduler(nesterov, wd):
    """A 10-entry table for 12 steps: warm-up, then a decay every 5 steps (at steps 8 and 13), so the torch
    scheduler itself holds the table's last rate over steps 10 and 11, where the table clamps."""
    make = lambda opt: _step(opt, step_size=5)  # noqa: E731
    sched = LRSchedule.from_torch(make, BASE, 10)
    ours, theirs = _params(), _params()
    opt = FusedSGD(ours, lr=BASE, momentum=0.5, nesterov=nesterov, weight_decay=wd)
    opt.set_lr_schedule(sched)
    ref = torch.optim.SGD(theirs, lr=BASE, momentum=0.5, nesterov=nesterov, weight_decay=wd)
    rs = make(ref)
    for t in range(12):
        _set_grads(ours, t)
        _set_grads(theirs, t)
        assert opt.state_dict()["param_groups"][0]["lr"] == sched.current_lr()
        opt.step()
        ref.step()
        rs.step()
    assert sched.position() == 12
    for a, b in zip(ours, theirs):
        torch.testing.assert_close(a, b)


def test_state_round_trip_continues_the_run():
    sched = LRSchedule.warmup_step(BASE, 2, 3, 0.5, 10)
    whole, first = _params(), _params()
    o_whole = FusedSGD(whole, lr=BASE, momentum=0.5)
    o_whole.set_lr_schedule(LRSchedule(sched.table))
    o_first = FusedSGD(first, lr=BASE, momentum=0.5)
    o_first.set_lr_schedule(sched)
    for t in range(7):
        for ps, o in ((whole, o_whole), (first, o_first)):
            if t < 5 or o is o_whole:
                _set_grads(ps, t)
                o.step()
    sd_opt, sd_sched = o_first.state_dict(), sched.state_dict()
    assert sd_sched["t"] == 5 and sd_opt["param_groups"][0]["lr"] == sched.current_lr() == sched.table[5].item()
    resumed = [p.detach().clone().requires_grad_() for p in first]
    o_res = FusedSGD(resumed, lr=123.0, momentum=0.5)
    fresh = LRSchedule.constant(1.0)
    fresh.load_state_dict(sd_sched)
    o_res.load_state_dict(sd_opt)
    o_res.set_lr_schedule(fresh)
    assert fresh.position() == 5 and torch.equal(fresh.table, sched.table)
    for t in (5, 6):
        _set_grads(resumed, t)
        o_res.step()
    for a, b in zip(resumed, whole):
        assert torch.equal(a, b)
    assert fresh.position() == 7


def _run(cmd):
    e = dict(os.environ)
    e.setdefault("CSED_AUTOBUILD", "0")
    return subprocess.run([sys.executable] + cmd, cwd=ROOT, capture_output=True, text=True, timeout=300, env=e)


def test_cli_writes_and_resumes_the_schedule(tmp_path):
    cmd = ["src/train.py", "--device", "cpu", "--synthetic", "--epochs", "1", "--train-size", "640", "--test-size",
           "200", "--no-plot", "--out-dir", str(tmp_path), "--lr", "0.05", "--lr-schedule", "warmup-cosine",
           "--warmup-steps", "3", "--lr-min", "0.001"]
    r = _run(cmd)
    assert r.returncode == 0, r.stderr[-2000:]
    path = tmp_path / "results" / "lr_schedule.pth"
    assert path.exists()
    sd = torch.load(path, weights_only=True)
    # 10 steps per epoch, checkpointed every 10 batches: written after step 0 of the only epoch
    want = LRSchedule.warmup_cosine(0.05, 3, 10, min_lr=0.001)
    assert torch.equal(sd["table"], want.table) and sd["t"] == 1
    osd = torch.load(tmp_path / "results" / "optimizer.pth", weights_only=True)
    assert osd["param_groups"][0]["lr"] == want.table[1].item()
    stock = torch.optim.SGD(torch.nn.ModuleList([torch.nn.Conv2d(1, 10, 5), torch.nn.Conv2d(10, 20, 5),
                                                 torch.nn.Linear(320, 50), torch.nn.Linear(50, 10)]).parameters(),
                            lr=0.01, momentum=0.5)
    stock.load_state_dict(osd)
    r = _run(cmd + ["--resume"])
    assert r.returncode == 0, r.stderr[-2000:]
    assert torch.load(path, weights_only=True)["t"] == 2  # continued from position 1, checkpointed after one more step
