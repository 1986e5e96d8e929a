"""Adam / AdamW where no GPU is needed: the fp64 oracle (tests/_adam_oracle.py) against torch.optim.Adam and
AdamW themselves, its derived bound against a plain float32 evaluation of the rule, the new op's and the
executor's argument lists, and the CLI on --device cpu.  (The op is registered for GPU tensors only: its
rejections run in tests/test_adam_gpu.py.)"""
import math
import os
import subprocess
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _adam_oracle as ado  # noqa: E402

from csed_514_project_distributed_training_using_pytorch_amd.engine import fused  # noqa: E402
from csed_514_project_distributed_training_using_pytorch_amd.models import Net  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LR, EPS = 1e-3, 1e-8


@pytest.mark.parametrize("betas", [(0.9, 0.999), (0.5, 0.9)], ids=lambda b: "b%g-%g" % b)
@pytest.mark.parametrize("wd", [0.0, 1e-2], ids=lambda w: "wd%g" % w)
@pytest.mark.parametrize("decoupled", [False, True], ids=["adam", "adamw"])
def test_oracle_equals_torch_in_fp64(decoupled, wd, betas):
    """Five fp64 steps of torch's optimizer and of the oracle from the same start, hyper-parameters that
    float32 holds exactly or rounded the way the oracle rounds them: 1e-12 relative, every step."""
    gen = torch.Generator().manual_seed(11)
    f = ado.f32
    hyper = dict(lr=f(LR), betas=(f(betas[0]), f(betas[1])), eps=f(EPS), weight_decay=f(wd))
    w = torch.nn.Parameter(torch.randn(257, generator=gen, dtype=torch.float64) * 0.25)
    opt = (torch.optim.AdamW if decoupled else torch.optim.Adam)([w], **hyper)
    p, m, v = w.detach().clone(), torch.zeros(257, dtype=torch.float64), torch.zeros(257, dtype=torch.float64)
    for t in range(1, 6):
        g = torch.randn(257, generator=gen, dtype=torch.float64)
        g[::7] = 0.0
        w.grad = g.clone()
        opt.step()
        p, m, v = ado.adam_reference(p, m, v, g, t, LR, betas, EPS, wd, decoupled)
        st = opt.state[w]
        for name, got, want in (("p", p, w.detach()), ("m", m, st["exp_avg"]), ("v", v, st["exp_avg_sq"])):
            err = ((got - want).abs() / want.abs().clamp_min(1e-300)).max().item()
            assert err <= 1e-12, f"step {t}: {name} differs from torch by {err:.3e} relative"
        assert float(st["step"]) == t


def _f32_rule(p, m, v, g, t, lr, betas, eps, wd, decoupled):
    """The rule in float32 torch operations, bias corrections as the kernels form them (float32 log(beta)
    from double, the product and expm1 in float32)."""
    f = lambda x: torch.tensor(x, dtype=torch.float32)  # noqa: E731
    lr, b1, b2, eps, wd = f(lr), f(betas[0]), f(betas[1]), f(eps), f(wd)
    one = f(1.0)
    if decoupled:
        p = p * (one - lr * wd)
    else:
        g = g + wd * p
    m = m + (one - b1) * (g - m)
    v = b2 * v + (one - b2) * (g * g)
    bc = [-torch.expm1(f(float(t)) * f(math.log(float(b)))) for b in (b1, b2)]
    p = p - (lr / bc[0]) * (m / (v.sqrt() / bc[1].sqrt() + eps))
    return p, m, v


@pytest.mark.parametrize("betas", [(0.9, 0.999), (0.5, 0.9)], ids=lambda b: "b%g-%g" % b)
@pytest.mark.parametrize("decoupled,wd", [(False, 0.0), (False, 1e-2), (True, 1e-2)], ids=["adam", "adam-wd", "adamw-wd"])
def test_float32_rule_stays_inside_the_bounds(decoupled, wd, betas):
    """A float32 evaluation of the rule (torch's CPU operations: correctly rounded, unfused) from random
    states with exact-zero gradients, zero moments and tiny second moments among them, at steps 1, 2, 3, 10
    and 1000: inside adam_bounds, which therefore ask nothing that the reference implementation alone
    misses; and the bounds are tight enough to mean something (without weight decay the parameter's is
    below 1e-5 of the step taken plus 4 u |p|)."""
    gen = torch.Generator().manual_seed(5)
    n = 4096
    for t in (1, 2, 3, 10, 1000):
        p = torch.randn(n, generator=gen) * 0.25
        g = torch.randn(n, generator=gen) * 10.0 ** torch.randint(-6, 2, (n,), generator=gen).float()
        m = torch.randn(n, generator=gen) * 0.1
        v = torch.rand(n, generator=gen) * 10.0 ** torch.randint(-12, 1, (n,), generator=gen).float()
        g[::5] = 0.0
        m[::3] = 0.0
        v[::15] = 0.0
        if t == 1:
            m.zero_(), v.zero_()
        got = _f32_rule(p, m, v, g, t, LR, betas, EPS, wd, decoupled)
        want = ado.adam_reference(p, m, v, g.double(), t, LR, betas, EPS, wd, decoupled)
        bounds = ado.adam_bounds(p, m, v, g.double(), t, LR, betas, EPS, wd, decoupled)
        for name, x, y, b in zip("mvp", (got[1], got[2], got[0]), (want[1], want[2], want[0]), bounds):
            err = (x.double() - y).abs()
            assert bool((err <= b).all()), f"t {t} {name}: worst error / bound {(err / b.clamp_min(1e-300)).max():.3f}"
        if wd == 0.0:  # (with weight decay g + wd p may cancel, and the bound rightly grows with it)
            moved = (want[0] - p.double()).abs()
            big = moved > 1e-6
            assert bool((bounds[2][big] <= 1e-5 * moved[big] + 4 * ado.U * p.double().abs()[big]).all()), f"t {t}: loose p bound"


def test_field_lists_and_schemas():
    from csed_514_project_distributed_training_using_pytorch_amd.ops import _native

    _native.require()  # (loads the extension: the schemas need no GPU)
    assert fused.ADAM_FIELDS == ("adam_v", "beta1", "beta2", "eps", "decoupled")
    assert fused.UPDATE_FIELDS[-2:] == ("ema", "ema_decay") and fused.UpdateArgs._fields == fused.UPDATE_FIELDS
    a = torch.ops.csed.lenet_update_adam.default._schema.arguments
    assert [x.name for x in a] == list(fused.UPDATE_FIELDS + fused.ADAM_FIELDS)
    assert [str(x.type) for x in a[-5:]] == ["Tensor", "float", "float", "float", "bool"]
    assert a[-5].alias_info is not None and a[-5].alias_info.is_write
    u = torch.ops.csed.lenet_update.default._schema.arguments
    assert [x.name for x in u] == list(fused.UPDATE_FIELDS), "lenet_update's schema is frozen"
    assert [str(x.type) for x in a[:len(u)]] == [str(x.type) for x in u]
    st = torch.classes.csed.LenetStepper()
    step = st._get_method("set_update_adam").schema.arguments
    assert [str(x.type) for x in step[1:]] == [str(x.type) for x in a]  # (a class method's schema has no names)
    assert len(st._get_method("set_update").schema.arguments) - 1 == len(fused.UPDATE_FIELDS)


def _run(cmd):
    e = dict(os.environ)
    e.setdefault("CSED_AUTOBUILD", "0")
    return subprocess.run([sys.executable] + cmd, cwd=ROOT, capture_output=True, text=True, timeout=300, env=e)


CLI = ["src/train.py", "--device", "cpu", "--synthetic", "--epochs", "1", "--train-size", "256", "--test-size", "64",
       "--no-plot"]


def test_cli_adam_on_cpu(tmp_path):
    r = _run(CLI + ["--out-dir", str(tmp_path), "--optimizer", "adam", "--lr", "0.001"])
    assert r.returncode == 0, r.stderr[-2000:]
    sd = torch.load(tmp_path / "results" / "optimizer.pth", weights_only=True)
    opt = torch.optim.Adam(Net().parameters())
    opt.load_state_dict(sd)
    assert set(sd["state"][0]) == {"step", "exp_avg", "exp_avg_sq"} and sd["param_groups"][0]["betas"] == (0.9, 0.999)
    # --resume with the other optimizer's file: a sentence, not a traceback
    r = _run(CLI + ["--out-dir", str(tmp_path), "--resume"])
    assert r.returncode != 0 and "Traceback" not in r.stderr and "optimizer" in r.stderr, r.stderr[-2000:]


def test_cli_rejects_bad_beta():
    r = _run(CLI + ["--optimizer", "adam", "--beta1", "1.0"])
    assert r.returncode != 0 and "--beta1" in r.stderr and "Traceback" not in r.stderr
