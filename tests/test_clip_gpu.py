"""csed::clip_grad_norm_ (csrc/kernels/clip.hip) against fp64 at the sizes where its two forms can go wrong, inside
guard floats, and inside a step of the fused engine (eager, graph-replayed) and of the per-op engine's optimizer.

``bound``, derived: the squares are non-negative, so the fp32 sum is off by at most one rounding per addition on
an element's way to the total (a thread's ceil(n / threads) fmafs, about log2(threads) butterfly and wave sums, G
partial sums) plus the square root's and the division's.  The tests allow twice it."""
import math

import pytest
import torch

from csed_514_project_distributed_training_using_pytorch_amd import ops
from csed_514_project_distributed_training_using_pytorch_amd.data import synthetic_mnist
from csed_514_project_distributed_training_using_pytorch_amd.engine.fused import FusedLeNetTrainer
from csed_514_project_distributed_training_using_pytorch_amd.engine.modular import ModularTrainer
from csed_514_project_distributed_training_using_pytorch_amd.models import Net
from csed_514_project_distributed_training_using_pytorch_amd.optim import FusedSGD, clip_plan

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
U = 2.0 ** -24
NP = 21840


def bound(n):
    p, threads = clip_plan(n), clip_plan(n).grid * clip_plan(n).threads
    return (math.ceil(n / threads) + math.log2(threads) + p.grid + 4) * U


def reference(g, max_norm):
    """(norm, coef, clipped g) in float64, from the fp32 values the kernel gets."""
    ref, m = g.double().cpu(), float(torch.tensor(max_norm, dtype=torch.float32))
    norm = ref.square().sum().sqrt().item()
    return norm, min(1.0, m / (norm + 1e-6)), ref * min(1.0, m / (norm + 1e-6))


def check_sgd_step(p0, p1, g, max_norm, norm_got):
    """A clipped SGD step (lr 0.1, momentum 0) against fp64: the norm; p0 - p1 = lr coef g within the clip's bound,
    the product's rounding and the new parameter's."""
    b, (norm, _, want) = 2 * bound(g.numel()), reference(g, max_norm)
    assert abs(norm_got - norm) <= b * norm
    p0, p1, want = p0.double().cpu(), p1.double().cpu(), want * float(torch.tensor(0.1, dtype=torch.float32))
    assert ((p0 - p1 - want).abs() <= (b + 3 * U) * want.abs() + U * torch.maximum(p0.abs(), p1.abs())).all()


def clip_in_guards(g, off, max_norm):
    """g clipped ``off`` floats past a 16-byte boundary of a fresh buffer between 1e30 / NaN guards: (values, stats)."""
    n, lo = g.numel(), 4 + off
    buf = torch.tensor([1e30, float("nan")], device=DEV).repeat((lo + n + 5) // 2)[:lo + n + 4].clone()
    guard = buf.view(torch.int32).clone()
    buf[lo:lo + n] = g
    stats, need = torch.zeros(2, device=DEV), clip_plan(n).partials
    torch.ops.csed.clip_grad_norm_(buf[lo:lo + n], max_norm, stats, torch.empty(need, device=DEV) if need else None)
    got = buf.view(torch.int32)
    assert torch.equal(got[:lo], guard[:lo]) and torch.equal(got[lo + n:], guard[lo + n:]), "guard floats changed"
    return buf[lo:lo + n].clone(), stats


@pytest.mark.parametrize("factor", [0.5, 2.0])
@pytest.mark.parametrize("off", [0, 1])
@pytest.mark.parametrize("n", [1, 3, 63, 64, 65, 4097, NP, "max", "max + 1", "3 * max + 5"], ids=str)
def test_kernel_against_fp64(n, off, factor):
    n = int(eval(n, {"max": clip_plan(1).one_wg_max})) if isinstance(n, str) else n
    g = torch.randn(n, generator=torch.Generator().manual_seed(n)).to(DEV)
    max_norm = factor * g.double().norm().item()
    norm, coef, want = reference(g, max_norm)
    out, stats = clip_in_guards(g, off, max_norm)
    b = 2 * bound(n)
    assert abs(stats[0].item() - norm) <= b * norm
    if factor > 1:
        assert stats[1].item() == 1.0 and torch.equal(out.view(torch.int32), g.view(torch.int32))
    else:
        assert abs(stats[1].item() - coef) <= (b + 2 * U) * coef
        assert ((out.double().cpu() - want).abs() <= (b + 2 * U) * want.abs()).all()
    again, stats2 = clip_in_guards(g, off, max_norm)  # (a fresh buffer, a second run: the same bits)
    assert torch.equal(again.view(torch.int32), out.view(torch.int32)) and torch.equal(stats2, stats)


def _engine(dtype, **kw):
    torch.manual_seed(1)
    eng = FusedLeNetTrainer(Net().to(DEV), synthetic_mnist(64, seed=3), global_batch=8, compute_dtype=dtype, **kw)
    eng.set_epoch_order(torch.arange(64))
    return eng


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32], ids=["bf16", "fp32"])
def test_fused_engine_steps(dtype):
    # (a) a clip that never bites: the split update with the clip in it trains bitwise like the one-kernel step
    plain, loose = _engine(dtype), _engine(dtype)
    assert len(plain._step_launches()) == 2 and plain.stepper() is not None
    loose.set_grad_clip(1e30)
    assert [name for name, _ in loose._step_launches()] == ["lenet_train", "lenet_update", "clip_grad_norm_",
                                                            "lenet_update"] and loose.stepper() is None
    for e in (plain, loose) * 3:
        e.step()
    assert torch.equal(plain.flat.data, loose.flat.data) and torch.equal(plain.momentum_buf, loose.momentum_buf)
    # (b) one clipped SGD step against fp64: p_before - p_after = lr * coef * g
    g = _engine(dtype).gradient()
    max_norm = 0.25 * g.double().norm().item()
    eager, replay = (_engine(dtype, lr=0.1, momentum=0.0) for _ in range(2))
    for e in (eager, replay):
        e.set_grad_clip(max_norm)
    p0 = eager.flat.data.clone()
    eager.step()
    check_sgd_step(p0, eager.flat.data, g, max_norm, eager.last_grad_norm())
    # (c) three graph-replayed steps are three eager steps, bit for bit
    eager.run_steps(2, use_graph=False)
    replay.run_steps(3, steps_per_graph=3)
    assert len(replay._graphs) == 1
    for a, c in zip(eager._state() + [eager.clip_stats], replay._state() + [replay.clip_stats]):
        assert torch.equal(a, c)
    for e in (plain, loose, eager, replay):
        e.close()


def test_per_op_engine_step(monkeypatch):
    """A clipped step against fp64, and against the unclipped one + torch's clip + SGD (twice the fp64 tolerance)."""
    monkeypatch.setattr(ops.rng.default_state, "device_step", None)  # (a trainer points it at its own step counter)
    gen = torch.Generator().manual_seed(7)
    x, t = torch.randn(8, 1, 28, 28, generator=gen).to(DEV, torch.bfloat16), torch.randint(0, 10, (8,), generator=gen).to(DEV)

    def trainer(max_norm):
        torch.manual_seed(1)
        tr = ModularTrainer(Net().to(DEV).train(), lr=0.1, momentum=0.0, graph=False, max_grad_norm=max_norm)
        p0 = tr.flat.data[:NP].clone()
        tr.train_batch(x, t)
        return tr, p0

    free, p0 = trainer(None)
    g = free.flat.grad[:NP].clone()
    max_norm = 0.25 * g.double().norm().item()
    clipped, _ = trainer(max_norm)
    check_sgd_step(p0, clipped.flat.data[:NP], g, max_norm, clipped.last_grad_norm())
    p = torch.nn.Parameter(p0.clone())
    p.grad = g.clone()
    torch.nn.utils.clip_grad_norm_([p], max_norm)
    torch.optim.SGD([p], lr=0.1).step()
    tol = 2 * ((2 * bound(NP) + 3 * U) * 0.1 * p.grad.abs() + U * torch.maximum(p0.abs(), p.detach().abs()))
    assert ((clipped.flat.data[:NP] - p.detach()).abs() <= tol).all()


def test_optimizer_large_form():
    """The two-launch form from Python, scratch sized by the plan (FusedSGD: optim.FusedAdam refuses GPU parameters)."""
    n = 100_000
    w = torch.nn.Parameter(torch.randn(n, generator=torch.Generator().manual_seed(2)).to(DEV))
    g = torch.randn(n, generator=torch.Generator().manual_seed(3)).to(DEV)
    opt = FusedSGD([w], lr=0.1, max_grad_norm=0.25 * g.double().norm().item())
    assert clip_plan(n).form == 1 and opt._clip.partials.numel() == clip_plan(n).partials
    p0, w.grad = w.detach().clone(), g.clone()
    opt.step()
    check_sgd_step(p0, w.detach(), g, opt.max_grad_norm, opt.last_grad_norm())
