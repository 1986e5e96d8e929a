"""The exponential moving average of the weights where no GPU is needed: FusedSGD's CPU rule against an
fp64 replay stacked on tests/_update_oracle.py's SGD reference, the argument lists and op schemas, and the
CLI on --device cpu.  (The ops themselves are registered for GPU tensors only, so the rejections of a bad
``ema`` argument -- dtype, length, device, decay, reduce-only -- run in tests/test_ema_gpu.py.)"""
import os
import subprocess
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _update_oracle as orc  # noqa: E402
from _update_oracle import LR, SGD_TABLE  # noqa: E402

from csed_514_project_distributed_training_using_pytorch_amd.engine import fused  # noqa: E402
from csed_514_project_distributed_training_using_pytorch_amd.models import Net  # noqa: E402
from csed_514_project_distributed_training_using_pytorch_amd.optim import FusedSGD  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -24


@pytest.mark.parametrize("hyper", SGD_TABLE, ids=lambda h: "m%g-d%g-wd%g-%s" % (h[0], h[1], h[2], "nag" if h[3] else "std"))
def test_fused_sgd_cpu_rule_matches_fp64(hyper):
    """Three CPU steps with set_ema(0.9): parameters within sgd_bounds of one fp64 step from the optimizer's
    own state, the average within (1 - d) P + 4 u (|e_old| + |p_new|) of the fp64 rule (the torch form
    rounds p - e, 1 - d, the product and the sum: four roundings of terms no larger than |e_old| + |p_new|)."""
    mom, damp, wd, nesterov = hyper
    d = 0.9
    gen = torch.Generator().manual_seed(3)
    params = [(torch.randn(s, generator=gen) * 0.25).requires_grad_() for s in ((7, 5), (13,), (3, 2, 2))]
    opt = FusedSGD(params, lr=LR, momentum=mom, dampening=damp, weight_decay=wd, nesterov=nesterov)
    assert opt.ema_flat is None
    opt.set_ema(d)
    assert torch.equal(opt.ema_flat, opt.flat.data) and opt.ema_flat.data_ptr() != opt.flat.data.data_ptr()
    n = opt.flat.numel
    for k in range(3):
        g = torch.randn(opt.flat.data.numel(), generator=gen)
        for i, p in enumerate(params):
            p.grad = opt.flat.view(g, i).clone()
        p0, m0, e0 = opt.flat.data.clone(), opt.momentum_flat.clone(), opt.ema_flat.clone()
        mz = torch.zeros_like(m0) if (k == 0 or mom == 0) else m0
        opt.step()
        p_ref, _ = orc.sgd_reference(p0, mz, g.double(), k == 0, LR, mom, damp, wd, nesterov)
        _, bp = orc.sgd_bounds(p0, mz, g.double(), LR, mom, wd)
        assert bool(((opt.flat.data.double() - p_ref).abs() <= bp)[:n].all()), f"step {k}: parameters"
        e_ref = e0.double() + (1.0 - orc.f32(d)) * (p_ref - e0.double())
        bound = (1.0 - orc.f32(d)) * bp + 4 * U * (e0.double().abs() + p_ref.abs())
        err = (opt.ema_flat.double() - e_ref).abs()
        assert bool((err <= bound)[:n].all()), f"step {k}: ema, worst error / bound {(err / bound)[:n].max():.3f}"
        assert not torch.equal(opt.ema_flat[:n], e0[:n])
    opt.set_param_names(["a", "b", "c"])
    sd = opt.ema_state_dict()
    assert list(sd) == ["a", "b", "c"] and all(sd[k].shape == p.shape for k, p in zip("abc", params))
    before = opt.ema_flat.clone()
    opt.ema_flat.zero_()
    opt.load_ema_state_dict(sd)
    assert torch.equal(opt.ema_flat[:n], before[:n])
    opt.set_ema(None)
    assert opt.ema_flat is None
    with pytest.raises(ValueError):
        opt.set_ema(1.0)


def test_field_lists_and_schemas():
    from csed_514_project_distributed_training_using_pytorch_amd.ops import _native

    _native.require()  # (loads the extension: the schemas need no GPU)
    kw = {f: None for f in fused.UPDATE_FIELDS[:-2]}
    args = fused.UpdateArgs(**kw)
    assert args.ema is None and args.ema_decay == 0.0
    assert fused.UPDATE_FIELDS[-2:] == ("ema", "ema_decay")
    for op in (torch.ops.csed.lenet_update,):
        a = op.default._schema.arguments
        assert [x.name for x in a[-2:]] == ["ema", "ema_decay"]
        assert str(a[-2].type) == "Optional[Tensor]" and a[-2].default_value is None and a[-2].has_default_value()
        assert str(a[-1].type) == "float" and a[-1].default_value == 0.0
    step = torch.classes.csed.LenetStepper()._get_method("set_update").schema.arguments
    assert [str(x.type) for x in step[-2:]] == ["Optional[Tensor]", "float"]  # (a class method's schema has no names)
    assert len(step) - 1 == len(fused.UPDATE_FIELDS)


def _run(cmd):
    e = dict(os.environ)
    e.setdefault("CSED_AUTOBUILD", "0")
    return subprocess.run([sys.executable] + cmd, cwd=ROOT, capture_output=True, text=True, timeout=300, env=e)


@pytest.mark.parametrize("script", ["src/train.py", "src/train_dist.py"])
def test_cli_ema_on_cpu(tmp_path, script):
    single = script == "src/train.py"
    cmd = [script, "--device", "cpu", "--synthetic", "--epochs", "1", "--train-size", "256", "--test-size", "64",
           "--no-plot"]
    off, on = tmp_path / "off", tmp_path / "on"
    r = _run(cmd + ["--out-dir", str(off)])
    assert r.returncode == 0, r.stderr[-2000:]
    assert "EMA weights" not in r.stdout
    assert not list(off.rglob("ema.*")), "an ema file without --ema-decay"
    r = _run(cmd + ["--out-dir", str(on), "--ema-decay", "0.9"])
    assert r.returncode == 0, r.stderr[-2000:]
    ema_path, model_path = (on / "results" / "ema.pth", on / "results" / "model.pth") if single else (on / "ema.pt", on / "model.pt")
    assert ema_path.exists() and model_path.exists()
    lines = r.stdout.splitlines()
    marks = [i for i, ln in enumerate(lines) if ln.startswith("EMA weights (decay 0.9): Avg. loss: ")]
    assert len(marks) == (2 if single else 1), r.stdout[-2000:]  # (train.py also tests before the first epoch)
    for i in marks:  # each right behind a validation line of the reference's format
        prev = [ln for ln in lines[:i] if ln.strip()][-1]
        assert prev.startswith("Test set: Avg. loss:" if single else "Epoch=")
    ema, model = torch.load(ema_path, weights_only=True), torch.load(model_path, weights_only=True)
    net = Net()
    net.load_state_dict(ema)
    assert list(ema) == list(model)
    assert any(not torch.equal(ema[k], model[k]) for k in ema), "the average equals the raw weights"
    if single:
        # --resume restores results/ema.pth: a recognisable average (every logit the fc2 bias, class 0 a
        # hundred ahead: a loss near 90) must be what the first EMA line, before any step, evaluates
        marked = {k: torch.zeros_like(v) for k, v in ema.items()}
        marked["fc2.bias"][0] = 100.0
        torch.save(marked, ema_path)
        r = _run(cmd + ["--out-dir", str(on), "--ema-decay", "0.9", "--resume"])
        assert r.returncode == 0, r.stderr[-2000:]
        first = [ln for ln in r.stdout.splitlines() if ln.startswith("EMA weights")][0]
        assert float(first.split("Avg. loss: ")[1].split(",")[0]) > 10.0, first
    r = _run(cmd + ["--out-dir", str(off), "--ema-decay", "1.0"])
    assert r.returncode != 0 and "--ema-decay" in r.stderr
