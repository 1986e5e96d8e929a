"""csed::augment_elastic (csrc/kernels/augment_elastic.hip) against tests/_elastic_oracle.py.  dst is pre-filled with
a sentinel byte.  Bounds, derived and not measured: the drawn field is two fp32 products of at most 28 nonzero terms
plus one scaling, |U| <= 1 and the rows of G sum to <= 1, so gamma_58 = 58 * 2^-24 < 2^-18, doubled for the MFMA's
summation order: |disp_out - D| <= 2^-17 alpha.  The bytes, against the float64 value v at the kernel's own theta_out
and disp_out: three fp32 roundings of a coordinate below 32 are <= 3 * 2^-20 px per axis, at <= 255 grey levels per
pixel on two axes <= 1.5e-3: |out - v| - 0.5 <= 2^-9."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _augment_oracle as ao  # noqa: E402
import _elastic_oracle as eo  # noqa: E402
from test_augment_gpu import _op as _affine  # noqa: E402  (dst, theta_out) of one csed::augment_affine launch

from csed_514_project_distributed_training_using_pytorch_amd.data import DeviceLoader, ElasticAugment, synthetic_mnist  # noqa: E402
from csed_514_project_distributed_training_using_pytorch_amd.engine.fused import FusedLeNetTrainer  # noqa: E402
from csed_514_project_distributed_training_using_pytorch_amd.ops import _native  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
SENTINEL = 0xA5
MAXIMA = (2.0, 15.0, 0.1)
IDENTITY = (1, 0, 0, 0, 1, 0)


def _op(src, idx=None, theta=None, disp=None, sigma=4.0, seed=0, epoch=0, maxima=(0.0, 0.0, 0.0), alpha=0.0):
    """(dst, theta_out, disp_out) on the host of one launch on ``src`` (uint8 numpy [N, 784])."""
    _native.require()
    s = torch.from_numpy(src).to(DEV)
    dst = torch.full_like(s, SENTINEL)
    idx = None if idx is None else torch.as_tensor(idx, dtype=torch.long, device=DEV)
    M = src.shape[0] if idx is None else idx.numel()
    tin = None if theta is None else torch.as_tensor(theta, dtype=torch.float32, device=DEV)
    din = None if disp is None else torch.as_tensor(disp, dtype=torch.float32, device=DEV)
    tout, dout = torch.full((M, 6), float("nan"), device=DEV), torch.full((M, 2, 28, 28), float("nan"), device=DEV)
    torch.ops.csed.augment_elastic(s, dst, idx, tin, tout, din, dout, torch.from_numpy(eo.gauss(sigma)).to(DEV),
                                   seed, epoch, *maxima, alpha)
    return dst.cpu().numpy(), tout.cpu().numpy(), dout.cpu().numpy()


@pytest.mark.parametrize("M", [1, 4, 5])
@pytest.mark.parametrize("shift", [(0, 0), (1, 0), (0, -3)], ids=["zero", "x+1", "y-3"])
def test_exact_fields(shift, M):
    src = ao.rows(M)
    theta = np.array([IDENTITY] * M, dtype=np.float32)
    disp = np.zeros((M, 2, 28, 28), dtype=np.float32)
    disp[:, 0], disp[:, 1] = shift
    got, tout, dout = _op(src, theta=theta, disp=disp)
    assert np.array_equal(tout, theta) and np.array_equal(dout, disp)
    assert np.array_equal(got, eo.warp(src, theta, disp))
    theta[:, 2], theta[:, 5] = shift  # the same integer shift as an affine map
    assert np.array_equal(got, _affine(src, theta=theta)[0])
    assert shift != (0, 0) or np.array_equal(got, src)


@pytest.mark.parametrize("idx", [[1, 4, 7, 10], [10, 7, 4, 1]], ids=["subset", "reversed"])
def test_idx_forms(idx):
    src, rows = ao.rows(12), np.array(idx)
    theta = np.array([IDENTITY] * 4, dtype=np.float32)
    disp = np.zeros((4, 2, 28, 28), dtype=np.float32)
    disp[:, 0], disp[:, 1] = (rows % 3 - 1)[:, None, None], (rows % 2)[:, None, None]  # (position i maps row idx[i])
    want = np.full_like(src, SENTINEL)
    want[rows] = eo.warp(src[rows], theta, disp)
    assert np.array_equal(_op(src, idx=idx, theta=theta, disp=disp)[0], want)


@pytest.mark.parametrize("alpha", [8.0, 34.0])
@pytest.mark.parametrize("sigma", [1.0, 4.0, 12.0])
@pytest.mark.parametrize("M", [1, 4, 5])
def test_drawn_field_and_bytes(M, sigma, alpha):
    src, seed, epoch = ao.rows(M + 3, seed=2), 0xABCDEF012345, 7
    idx = np.arange(M + 2, 2, -1)  # M rows, the all-255 last row among them
    got, tout, dout = _op(src, idx=idx, sigma=sigma, seed=seed, epoch=epoch, maxima=MAXIMA, alpha=alpha)
    err = float(np.abs(dout - eo.draw_disp(idx, seed, epoch, alpha, eo.gauss(sigma))).max())
    print(f"M {M} sigma {sigma} alpha {alpha}: worst |disp_out - D| = {err:.3e} (bound {2.0 ** -17 * alpha:.3e})")
    assert err <= 2.0 ** -17 * alpha
    assert np.array_equal(tout, _affine(src, idx=idx, seed=seed, epoch=epoch, maxima=MAXIMA)[1])
    berr = float(np.abs(got[idx] - eo.warp_value(src[idx], tout, dout)).max() - 0.5)
    print(f"M {M} sigma {sigma} alpha {alpha}: worst |out - v| - 0.5 = {berr:.3e} (bound {2.0 ** -9:.3e})")
    assert berr <= 2.0 ** -9
    assert (np.delete(got, idx, 0) == SENTINEL).all()


def test_draws_are_keyed_by_row_and_epoch():
    src, idx, kw = ao.rows(40, seed=2), np.array([33, 2, 17, 39, 8, 21]), dict(seed=3, maxima=MAXIMA, alpha=34.0)
    got = _op(src, idx=idx, epoch=0, **kw)[0]
    assert np.array_equal(_op(src, idx=idx[::-1].copy(), epoch=0, **kw)[0][idx], got[idx])
    assert np.array_equal(_op(src, epoch=0, **kw)[0][idx], got[idx])
    assert not np.array_equal(_op(src, idx=idx, epoch=1, **kw)[0][idx], got[idx])


def _direct(images, order):
    """The op applied directly: what an engine's buffer must hold at the rows of ``order`` after its first epoch."""
    dst = torch.full_like(images, SENTINEL)
    ElasticAugment(34.0, 4.0, max_shift=2, seed=1).apply(images, dst, idx=order)
    return dst[order]


def test_fused_engine_trains_on_the_elastic_copy():
    order = torch.arange(63, 15, -1)  # 48 of the 64 rows
    eng, plain = FusedLeNetTrainer.smoke_instance(DEV), FusedLeNetTrainer.smoke_instance(DEV)
    before, dorder = eng.train_data.images.clone(), order.to(DEV)
    aug = ElasticAugment(34.0, 4.0, max_shift=2, seed=1)
    eng.set_augment(aug)
    eng.set_epoch_order(order)
    assert aug.epoch == 1 and torch.equal(eng.train_images[dorder], _direct(before, dorder))
    assert torch.equal(eng.train_images[:16], before[:16]) and not torch.equal(eng.train_images[dorder], before[dorder])
    eng.run_steps(1)  # one graph-replayed step on the deformed rows
    assert np.isfinite(eng.take_loss()[0])
    eng.set_augment(None)  # switched off again: a step from the same state is the plain engine's, bit for bit
    for e in (eng, plain):
        e.flat.data.copy_(plain.flat.data)
        for t in (e.momentum_buf, e.step_count, e.rng_offset):
            t.zero_()
        e.repack()
        e.set_epoch_order(order)
        e.run_steps(1)
    assert eng.train_images.data_ptr() == eng.train_data.images.data_ptr()
    assert torch.equal(eng.flat.data, plain.flat.data) and eng.take_loss() == plain.take_loss()


def test_device_loader_gathers_from_the_elastic_copy():
    data = synthetic_mnist(64, seed=3)
    loader = DeviceLoader(data, 16, device=DEV, augment=ElasticAugment(34.0, 4.0, max_shift=2, seed=1))
    next(iter(loader))
    assert torch.equal(loader.images, _direct(loader.data.images, torch.arange(64, device=DEV)))
    assert torch.equal(loader.data.images, data.images.to(DEV))
