"""csed::augment_stroke (csrc/kernels/augment_stroke.hip) against tests/_stroke_oracle.py, bit for bit.  dst is
pre-filled with a sentinel byte, so a row not written or written elsewhere fails."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _stroke_oracle as so  # noqa: E402

from csed_514_project_distributed_training_using_pytorch_amd.data import AffineAugment, DeviceLoader, StrokeAugment, synthetic_mnist  # noqa: E402
from csed_514_project_distributed_training_using_pytorch_amd.engine.fused import FusedLeNetTrainer  # noqa: E402
from csed_514_project_distributed_training_using_pytorch_amd.ops import _native  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)


def _op(src, params=None, idx=None, in_place=False, seed=0, epoch=0, knobs=(0.0, 0.0, 1, 28)):
    """(dst, params_out) on the host of one launch on uint8 NumPy ``src``; dst is pre-filled with SENTINEL, or is src."""
    _native.require()
    s = torch.from_numpy(src).to(DEV)
    dst = s if in_place else torch.full_like(s, so.SENTINEL)
    idx = None if idx is None else torch.as_tensor(idx, dtype=torch.long, device=DEV)
    pin = None if params is None else torch.tensor(params, dtype=torch.int32, device=DEV)
    pout = torch.full((s.shape[0] if idx is None else idx.numel(), 6), -99, dtype=torch.int32, device=DEV)
    torch.ops.csed.augment_stroke(s, dst, idx, pin, pout, seed, epoch, *knobs)
    return dst.cpu().numpy(), pout.cpu().numpy()


@pytest.mark.parametrize("case", list(so.EXPLICIT))
def test_explicit_parameters(case):
    src, params = so.EXPLICIT[case]
    assert all(np.array_equal(g, w) for g, w in zip(_op(src, params), so.apply(src, params)))


@pytest.mark.parametrize("idx", [None, [7, 2, 5, 0, 8, 3], [4, -1, 6, 9, 1]], ids=["all", "permuted", "outside"])
def test_idx_forms_and_in_place(idx):
    src = np.random.default_rng(4).integers(0, 256, (9, 784), dtype=np.uint8)  # N = 9: index 9 is outside
    at = np.arange(9) if idx is None else np.array(idx)
    params, ok = np.array([(100 * i - 300, i % 2, i, 2, 9, 30) for i in range(at.size)]), (at >= 0) & (at < 9)
    want, kept = np.full_like(src, so.SENTINEL), src.copy()
    want[at[ok]] = kept[at[ok]] = so.apply(src[at[ok]], params[ok])[0]
    assert np.array_equal(_op(src, params.tolist(), idx)[0], want)
    assert np.array_equal(_op(src, params.tolist(), idx, in_place=True)[0], kept)  # dst is src, idx distinct


@pytest.mark.parametrize("epoch", [0, 3])
@pytest.mark.parametrize("seed", [3, 0xABCDEF012345])
def test_drawn_parameters(seed, epoch):
    small, far = np.random.default_rng(6).integers(0, 256, (8, 784), dtype=np.uint8), np.array([0, 1, 59_999, 31_337])
    big = torch.randint(0, 256, (60_000, 784), dtype=torch.uint8).numpy()
    want = so.draw(np.concatenate([np.arange(8), far]), seed, epoch, *so.DRAWN)
    assert (want[:, 0] > 0).any() and (want[:, 0] < 0).any() and set(want[:, 1]) == {0, 1}  # the seeds were picked for this
    got, used = _op(small, seed=seed, epoch=epoch, knobs=so.DRAWN)
    assert np.array_equal(used, want[:8]) and np.array_equal(got, so.apply(small, want[:8])[0])
    got, used = _op(big, idx=far, seed=seed, epoch=epoch, knobs=so.DRAWN)
    assert np.array_equal(used, want[8:]) and np.array_equal(got[far], so.apply(big[far], want[8:])[0])
    aug = StrokeAugment(*so.DRAWN[:2], so.DRAWN[2:], seed=seed)
    aug.epoch = epoch
    assert np.array_equal(aug.draw(torch.from_numpy(far)).numpy(), want[8:])


@pytest.mark.parametrize("consumer", ["fused", "loader"])
def test_engines_train_on_affine_then_stroke(consumer):
    data, s = synthetic_mnist(64, seed=3), 7  # (smoke_instance's train set)
    aug = StrokeAugment(1.5, 0.5, inner=AffineAugment(2.0, seed=s), seed=s)
    if consumer == "fused":
        eng, order = FusedLeNetTrainer.smoke_instance(DEV), torch.randperm(64)
        eng.set_augment(aug)
        start, images = (lambda: eng.set_epoch_order(order)), (lambda: eng.train_images)
    else:
        loader, order = DeviceLoader(data, 16, device=DEV, augment=aug), torch.arange(64)
        start, images = (lambda: next(iter(loader))), (lambda: loader.images)
    plain, affine, seen = data.images.to(DEV), AffineAugment(2.0, seed=s), []
    for epoch in (0, 1):  # each epoch start: the stroke oracle on AffineAugment's own output for that epoch
        start()
        affine.epoch, warped = epoch, torch.full_like(plain, so.SENTINEL)
        affine.apply(plain, warped, idx=order.to(DEV))
        want = so.apply(warped[order].cpu().numpy().reshape(-1, 784), so.draw(order.numpy(), s, epoch, 1.5, 0.5, 4, 12))[0]
        seen.append(images()[order].cpu().numpy().reshape(-1, 784))
        assert aug.epoch == epoch + 1 and np.array_equal(seen[-1], want)
    assert not np.array_equal(seen[0], seen[1])
