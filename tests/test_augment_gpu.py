"""csed::augment_affine (csrc/kernels/augment.hip) against tests/_augment_oracle.py: exact maps bit for bit at the
workgroup's edges, every idx form, general and drawn maps within tau of the float64 value, and both engines'
augmented buffers.  dst is pre-filled with a sentinel byte, so a row not written or written elsewhere fails.
Bounds: 4x the worst figure measured on an MI355X against the float64 oracle, rounded up to a power of two (as in
tests/test_elementwise_oracle_gpu.py; each test prints its figure before it asserts).  TAU: worst |out - v| - 0.5
was 1.47e-5 (the general maps).  THETA_REL: worst |theta_out - theta64| / |theta64| was 1.17e-7."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _augment_oracle as ao  # noqa: E402

from csed_514_project_distributed_training_using_pytorch_amd.data import AffineAugment, DeviceLoader, synthetic_mnist  # noqa: E402
from csed_514_project_distributed_training_using_pytorch_amd.engine.fused import FusedLeNetTrainer  # noqa: E402
from csed_514_project_distributed_training_using_pytorch_amd.ops import _native  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
TAU, THETA_REL = 2.0 ** -14, 2.0 ** -21
SENTINEL = 0xA5
MAXIMA = (2.0, 15.0, 0.1)


def _op(src, idx=None, theta=None, seed=0, epoch=0, maxima=(0.0, 0.0, 0.0)):
    """(dst, theta_out) on the host of one launch on ``src`` (uint8 numpy [N, 784]), dst pre-filled with SENTINEL."""
    _native.require()
    s = torch.from_numpy(src).to(DEV)
    dst = torch.full_like(s, SENTINEL)
    idx = None if idx is None else torch.as_tensor(idx, dtype=torch.long, device=DEV)
    M = src.shape[0] if idx is None else idx.numel()
    tin = None if theta is None else torch.as_tensor(theta, dtype=torch.float32, device=DEV)
    tout = torch.full((M, 6), float("nan"), device=DEV)
    torch.ops.csed.augment_affine(s, dst, idx, tin, tout, seed, epoch, *maxima)
    return dst.cpu().numpy(), tout.cpu().numpy()


def _within_tau(out, v, what):
    err = float(np.abs(out - v).max() - 0.5)
    print(f"{what}: worst |out - v| - 0.5 = {err:.3e} (tau {TAU:.3e})")
    assert err <= TAU, f"{what}: {err:.3e} above tau {TAU:.3e}"


@pytest.mark.parametrize("M", [1, 3, 4, 5, 9])
@pytest.mark.parametrize("name", list(ao.EXACT))
def test_exact_maps(name, M):
    src = ao.rows(M)
    theta = np.array([ao.EXACT[name]] * M, dtype=np.float32)
    got, tout = _op(src, theta=theta)
    assert np.array_equal(got, ao.warp(src, theta)) and np.array_equal(tout, theta)
    want = {"identity": src, "gone": np.zeros_like(src),
            "turn90": np.rot90(src.reshape(M, 28, 28), -1, (1, 2)).reshape(M, 784)}.get(name)
    assert want is None or np.array_equal(got, want)


@pytest.mark.parametrize("idx", [None, [1, 4, 7, 10], [10, 7, 4, 1], [2, 5, 5, 9]], ids=["all", "strided", "reversed", "dup"])
def test_idx_forms(idx):
    src = ao.rows(12)
    rows = np.arange(12) if idx is None else np.array(idx)
    theta = np.array([(1, 0, r % 3 - 1, 0, 1, r % 2) for r in rows], dtype=np.float32)  # (position i maps row idx[i])
    want = np.full_like(src, SENTINEL)
    want[rows] = ao.warp(src[rows], theta)
    assert np.array_equal(_op(src, idx=idx, theta=theta)[0], want)


def test_general_maps():
    g, M = np.random.default_rng(17), 64
    src = ao.rows(M, seed=9)
    phi, s = np.radians(g.uniform(-20, 20, M)), g.uniform(0.8, 1.25, M)
    theta = np.stack([np.cos(phi) / s, np.sin(phi) / s, g.uniform(-4, 4, M), -np.sin(phi) / s, np.cos(phi) / s,
                      g.uniform(-4, 4, M)], 1).astype(np.float32)
    _within_tau(_op(src, theta=theta)[0], ao.warp_value(src, theta), "general maps")


@pytest.mark.parametrize("epoch", [0, 7])
@pytest.mark.parametrize("seed", [3, 0xABCDEF012345])
def test_drawn_maps(seed, epoch):
    src, idx = ao.rows(40, seed=2), np.array([33, 2, 17, 39, 8, 21])
    got, tout = _op(src, idx=idx, seed=seed, epoch=epoch, maxima=MAXIMA)
    want = ao.draw_theta(idx, seed, epoch, *MAXIMA)
    rel = float((np.abs(tout - want) / np.abs(want)).max())
    print(f"drawn maps seed {seed} epoch {epoch}: worst relative theta error {rel:.3e} (bound {THETA_REL:.3e})")
    assert rel <= THETA_REL
    _within_tau(got[idx], ao.warp_value(src[idx], tout), f"drawn maps seed {seed} epoch {epoch}")
    assert (np.delete(got, idx, 0) == SENTINEL).all()
    # keyed by the dataset row: another order of the same rows, and no idx at all, give the same bytes
    assert np.array_equal(_op(src, idx=idx[::-1].copy(), seed=seed, epoch=epoch, maxima=MAXIMA)[0][idx], got[idx])
    assert np.array_equal(_op(src, seed=seed, epoch=epoch, maxima=MAXIMA)[0][idx], got[idx])
    assert not np.array_equal(_op(src, idx=idx, seed=seed, epoch=epoch + 1, maxima=MAXIMA)[0][idx], got[idx])


def _direct(images, order):
    """The op applied directly: what an engine's buffer must hold at the rows of ``order`` after its first epoch."""
    dst = torch.full_like(images, SENTINEL)
    AffineAugment(max_shift=2, seed=1).apply(images, dst, idx=order)
    return dst[order]


def test_fused_engine_trains_on_the_augmented_copy():
    order = torch.arange(63, 15, -1)  # 48 of the 64 rows
    eng, plain = FusedLeNetTrainer.smoke_instance(DEV), FusedLeNetTrainer.smoke_instance(DEV)
    before, dorder = eng.train_data.images.clone(), order.to(DEV)
    aug = AffineAugment(max_shift=2, seed=1)
    eng.set_augment(aug)
    eng.set_epoch_order(order)
    assert aug.epoch == 1 and torch.equal(eng.train_images[dorder], _direct(before, dorder))
    assert torch.equal(eng.train_images[:16], before[:16]) and not torch.equal(eng.train_images[dorder], before[dorder])
    assert torch.equal(eng.train_data.images, before)
    eng.run_steps(1)  # one graph-replayed step on the augmented rows
    assert np.isfinite(eng.take_loss()[0])
    # switched off again: a step from the same state is the plain engine's, bit for bit
    eng.set_augment(None)
    for e in (eng, plain):
        e.flat.data.copy_(plain.flat.data)
        for t in (e.momentum_buf, e.step_count, e.rng_offset):
            t.zero_()
        e.repack()
        e.set_epoch_order(order)
        e.run_steps(1)
    assert eng.train_images.data_ptr() == eng.train_data.images.data_ptr()
    assert torch.equal(eng.flat.data, plain.flat.data) and eng.take_loss() == plain.take_loss()


def test_device_loader_gathers_from_the_augmented_copy():
    data = synthetic_mnist(64, seed=3)
    loader = DeviceLoader(data, 16, device=DEV, augment=AffineAugment(max_shift=2, seed=1))
    x, _ = next(iter(loader))
    order = torch.arange(64, device=DEV)
    assert torch.equal(loader.images, _direct(loader.data.images, order))
    assert torch.equal(loader.data.images, data.images.to(DEV))
    assert not torch.equal(x, DeviceLoader(data, 16, device=DEV).batch(order[:16])[0])
