"""data.StrokeAugment where no GPU is needed: its CPU path against tests/_stroke_oracle.py bit for bit, and the CLI."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _stroke_oracle as so  # noqa: E402

from csed_514_project_distributed_training_using_pytorch_amd.data import AffineAugment, StrokeAugment  # noqa: E402
from csed_514_project_distributed_training_using_pytorch_amd.engine.cli import single_main  # noqa: E402


@pytest.mark.parametrize("case", list(so.EXPLICIT))
def test_cpu_explicit_parameters(case):
    src, params = so.EXPLICIT[case]
    dst = torch.full((src.shape[0], 784), so.SENTINEL, dtype=torch.uint8)
    used = StrokeAugment().apply(torch.from_numpy(src), dst, params=torch.tensor(params, dtype=torch.int32), return_params=True)
    assert all(np.array_equal(g.numpy(), w) for g, w in zip((dst, used), so.apply(src, params)))


@pytest.mark.parametrize("kw", [dict(max_thickness=3.5), dict(erase_p=1.5), dict(erase_size=(0, 4)),
                                dict(erase_size=(9, 4)), dict(max_thickness=float("nan")), dict(erase_p=float("nan"))])
def test_constructor_rejects(kw):
    with pytest.raises(ValueError):
        StrokeAugment(**kw)


def test_drawn_parameters_and_composition_with_inner():
    src, inner, alone = torch.from_numpy(so.rows()), AffineAugment(max_shift=2, seed=5), AffineAugment(max_shift=2, seed=5)
    aug = StrokeAugment(0, 0, inner=inner)
    assert aug.enabled and not StrokeAugment().enabled and aug.seed == 5
    aug.epoch += 2
    alone.epoch = 2  # (the setter reaches inner: the same maps below)
    a, b, idx = torch.full_like(src, so.SENTINEL), torch.full_like(src, so.SENTINEL), torch.tensor([3, 1, 4])
    aug.apply(src, a, idx=idx)  # its own part off: what inner writes
    alone.apply(src, b, idx=idx)
    assert inner.epoch == 2 and torch.equal(a, b) and (a[0] == so.SENTINEL).all()
    on = StrokeAugment(*so.DRAWN[:2], so.DRAWN[2:], inner=inner, seed=9)  # on: the oracle on inner's output, one seed
    on.epoch = 3
    want = so.draw(idx.numpy(), 9, 3, *so.DRAWN)
    assert inner.seed == 9 and np.array_equal(on.draw(idx).numpy(), want)
    used = on.apply(src, a, idx=idx, return_params=True)
    inner.apply(src, b, idx=idx)
    assert np.array_equal(used.numpy(), want) and np.array_equal(a[idx].numpy(), so.apply(b[idx].numpy(), want)[0])


def test_cli_flags_on_cpu(tmp_path):
    base = ["--device", "cpu", "--synthetic", "--train-size", "128", "--test-size", "64", "--epochs", "1", "--no-plot",
            "--out-dir", str(tmp_path)]
    assert single_main(base + ["--augment-thickness", "1", "--augment-erase", "0.5"]) == 0
    with pytest.raises(SystemExit) as e:
        single_main(base + ["--augment-thickness", "4"])
    assert "--augment-thickness" in str(e.value) and "--augment-erase-size" in str(e.value)
