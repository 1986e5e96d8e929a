"""data.ElasticAugment where no GPU is needed: its CPU path against tests/_elastic_oracle.py under
tests/test_elastic_gpu.py's bounds, the constructor's checks, and the CLI flags on --device cpu."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _augment_oracle as ao  # noqa: E402
import _elastic_oracle as eo  # noqa: E402

from csed_514_project_distributed_training_using_pytorch_amd.data import AffineAugment, ElasticAugment  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("sigma", [1.0, 4.0, 12.0])
def test_cpu_path_against_the_oracle(sigma):
    src, idx, alpha = torch.from_numpy(ao.rows(8)), torch.tensor([7, 2, 5, 0]), 34.0
    aug = ElasticAugment(alpha, sigma, 2, 15, 0.1, seed=3)
    aug.epoch = 7
    dst = torch.full_like(src, 0xA5)
    theta, disp = aug.apply(src, dst, idx=idx, return_theta=True, return_disp=True)
    assert np.array_equal(aug.gauss("cpu").numpy(), eo.gauss(sigma))
    err = np.abs(disp.numpy() - eo.draw_disp(idx.numpy(), 3, 7, alpha, eo.gauss(sigma))).max()
    berr = np.abs(dst.numpy()[idx] - eo.warp_value(src.numpy()[idx], theta.numpy(), disp.numpy())).max() - 0.5
    print(f"cpu path sigma {sigma}: worst |disp - D| = {err:.3e}, worst |out - v| - 0.5 = {berr:.3e}")
    assert err <= 2.0 ** -17 * alpha and berr <= 2.0 ** -9
    affine = AffineAugment(2, 15, 0.1, seed=3)
    affine.epoch = 7
    assert torch.equal(theta, affine.draw(idx))  # the affine stream is untouched by the field's
    assert (np.delete(dst.numpy(), idx.numpy(), 0) == 0xA5).all()  # rows not named are not written


def test_alpha_zero_is_the_affine_augmenter_and_bad_values_raise():
    src = torch.from_numpy(ao.rows(5))
    a, b = torch.full_like(src, 0xA5), torch.full_like(src, 0xA5)
    assert not ElasticAugment(0).enabled and ElasticAugment(8).enabled and ElasticAugment(0, max_shift=1).enabled
    ElasticAugment(0, 4, 2, 15, 0.1, seed=3).apply(src, a)
    AffineAugment(2, 15, 0.1, seed=3).apply(src, b)
    assert torch.equal(a, b)
    for bad in (dict(alpha=-1), dict(alpha=float("inf")), dict(alpha=float("nan")), dict(alpha=8, sigma=0),
                dict(alpha=8, sigma=-2), dict(alpha=8, max_scale=1), dict(alpha=8, max_shift=-1)):
        with pytest.raises(ValueError):
            ElasticAugment(**bad)


@pytest.mark.parametrize("script", ["src/train.py", "src/train_dist.py"])
def test_cli_elastic_flags_on_cpu(script, tmp_path):
    e = dict(os.environ)
    e.setdefault("CSED_AUTOBUILD", "0")
    cmd = [sys.executable, script, "--device", "cpu", "--synthetic", "--epochs", "1", "--train-size", "256",
           "--test-size", "64", "--no-plot", "--out-dir", str(tmp_path)]
    on, bad = (subprocess.run(cmd + f, cwd=ROOT, capture_output=True, text=True, timeout=300, env=e)
               for f in (["--augment-elastic", "34", "--augment-shift", "2"], ["--augment-elastic-sigma", "0"]))
    assert on.returncode == 0 and "loss" in on.stdout.lower(), on.stderr[-2000:]
    assert bad.returncode != 0 and "--augment-elastic-sigma" in bad.stderr and "Traceback" not in bad.stderr
