"""data.AffineAugment where no GPU is needed: its CPU path against tests/_augment_oracle.py (the exact maps, then
drawn ones within tests/test_augment_gpu.py's tau), what keys the draws, and the CLI flags on --device cpu."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _augment_oracle as ao  # noqa: E402

from csed_514_project_distributed_training_using_pytorch_amd.data import AffineAugment  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TAU = 2.0 ** -14  # the GPU test's; this path evaluates the float32 maps in float64 like the oracle


@pytest.mark.parametrize("name", list(ao.EXACT))
def test_cpu_exact_maps(name):
    src = torch.from_numpy(ao.rows(5))
    theta = torch.tensor([ao.EXACT[name]] * 5, dtype=torch.float32)
    dst = torch.full_like(src, 0xA5)
    AffineAugment().apply(src, dst, theta=theta)
    assert torch.equal(dst, torch.from_numpy(ao.warp(src.numpy(), theta.numpy())))
    assert name != "identity" or torch.equal(dst, src)


def test_cpu_drawn_maps_within_tau_and_keyed_by_row():
    src = torch.from_numpy(ao.rows(24))
    aug = AffineAugment(max_shift=2, max_rot_deg=15, max_scale=0.1, seed=3)
    aug.epoch = 7
    idx = torch.tensor([20, 3, 11, 23, 3])
    dst = torch.full_like(src, 0xA5)
    theta = aug.apply(src, dst, idx=idx, return_theta=True)
    assert np.allclose(theta.numpy(), ao.draw_theta(idx.numpy(), 3, 7, 2, 15, 0.1), rtol=2.0 ** -22, atol=0)
    err = np.abs(dst.numpy()[idx] - ao.warp_value(src.numpy()[idx], theta.numpy())).max() - 0.5
    print(f"cpu path: worst |out - v| - 0.5 = {err:.3e}")
    assert err <= TAU
    assert (np.delete(dst.numpy(), idx.numpy(), 0) == 0xA5).all()  # rows not named are not written
    full = torch.full_like(src, 0xA5)
    aug.apply(src, full)  # the same rows through another order: the same bytes
    assert torch.equal(full[idx], dst[idx])
    aug.epoch = 8
    assert not torch.equal(aug.draw(idx), theta)  # another epoch, another seed: other maps
    aug.epoch, aug._seed = 7, 4
    assert not torch.equal(aug.draw(idx), theta)
    assert not AffineAugment().enabled and AffineAugment(max_scale=0.1).enabled


@pytest.mark.parametrize("script", ["src/train.py", "src/train_dist.py"])
def test_cli_augment_flags_on_cpu(script, tmp_path):
    e = dict(os.environ)
    e.setdefault("CSED_AUTOBUILD", "0")
    cmd = [sys.executable, script, "--device", "cpu", "--synthetic", "--epochs", "1", "--train-size", "256",
           "--test-size", "64", "--no-plot", "--out-dir", str(tmp_path)]
    flags = ["--augment-shift", "2", "--augment-rotate", "15", "--augment-scale", "0.1"]
    on, off, bad = (subprocess.run(cmd + f, cwd=ROOT, capture_output=True, text=True, timeout=300, env=e)
                    for f in (flags, [], ["--augment-scale", "1"]))
    assert on.returncode == 0 and off.returncode == 0, on.stderr[-2000:]
    out = [re.sub(r"time_elapsed=[0-9.]+", "", r.stdout) for r in (on, off)]
    assert "loss" in out[1].lower() and out[0] != out[1]  # the flags reached the trainer: other images, other losses
    assert bad.returncode != 0 and "--augment-scale" in bad.stderr and "Traceback" not in bad.stderr
