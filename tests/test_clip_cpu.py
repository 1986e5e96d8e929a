"""Gradient clipping of CPU parameters (optim, --clip-grad-norm --device cpu): torch's clip_grad_norm_, exactly."""
import inspect

import pytest
import torch

from csed_514_project_distributed_training_using_pytorch_amd.engine.cli import single_main
from csed_514_project_distributed_training_using_pytorch_amd.engine.modular import ModularTrainer
from csed_514_project_distributed_training_using_pytorch_amd.optim import FusedAdam, FusedSGD


@pytest.mark.parametrize("max_norm", [8.0, 128.0], ids=["clipped", "unclipped"])  # (the gradients' norm: about 32)
def test_cpu_sgd_equals_torch_clip_plus_sgd(max_norm):
    gen = torch.Generator().manual_seed(0)
    a = torch.nn.Parameter(torch.randn(1027, generator=gen))
    b = torch.nn.Parameter(a.detach().clone())
    kw = dict(lr=0.05, momentum=0.5)  # (where the two optimizers agree bit for bit unclipped)
    ours, theirs = FusedSGD([a], max_grad_norm=max_norm, **kw), torch.optim.SGD([b], **kw)
    for _ in range(3):
        g = torch.randn(1027, generator=gen)
        a.grad, b.grad = g.clone(), g.clone()
        want = torch.nn.utils.clip_grad_norm_([b], max_norm)
        ours.step()
        theirs.step()
        assert ours.last_grad_norm() == float(want) and torch.equal(a, b)


def test_defaults_are_off():
    for cls in (FusedSGD, FusedAdam, ModularTrainer):
        assert inspect.signature(cls.__init__).parameters["max_grad_norm"].default is None


@pytest.mark.parametrize("optimizer", ["sgd", "adam"])
def test_cli_clips_through_torch_on_cpu(tmp_path, monkeypatch, optimizer):
    calls, real = [], torch.nn.utils.clip_grad_norm_
    monkeypatch.setattr(torch.nn.utils, "clip_grad_norm_",
                        lambda params, m, *a, **k: calls.append(float(m)) or real(params, m, *a, **k))
    base = ["--device", "cpu", "--synthetic", "--train-size", "128", "--test-size", "64", "--epochs", "1", "--no-plot",
            "--batch-size", "32", "--optimizer", optimizer, "--out-dir", str(tmp_path)]
    assert single_main(base) == 0 and calls == []  # (flag absent: no clip)
    assert single_main(base + ["--clip-grad-norm", "0.5"]) == 0 and calls == [0.5] * 4  # (one per batch)
