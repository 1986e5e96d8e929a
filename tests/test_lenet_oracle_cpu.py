"""The fp64 oracle of one sample (tests/_lenet_oracle.py) against torch autograd, its pooling ties, the
pinned share of the candidate list and the rounding band E the GPU tests use (no GPU here)."""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _lenet_oracle as orc  # noqa: E402
from _lenet_oracle import BF16, CONV_SEGMENTS, FP16, FP32  # noqa: E402

from csed_514_project_distributed_training_using_pytorch_amd.models import Net  # noqa: E402


def _dt(dtype) -> str:
    return str(dtype).replace("torch.", "")


def _net64():
    torch.manual_seed(orc.WEIGHT_SEED)
    return Net().double()


def _torch_sample(net, x32, label, d2=None, d1=None, p=0.0):
    """ref src/model.py:15-22 in fp64 on one sample, the keep masks applied as tests/test_dropout_pin_gpu.py
    applies the host masks (_ref_forward_with_masks).  Returns (log-probs, loss, conv gradient [5280])."""
    s = 1.0 / (1.0 - p)
    x = torch.from_numpy(x32).double().view(1, 1, 28, 28)
    d2 = torch.ones(1, 20) if d2 is None else d2.view(1, 20)
    d1 = torch.ones(1, 50) if d1 is None else d1.view(1, 50)
    h = F.relu(F.max_pool2d(net.conv1(x), 2))
    y = net.conv2(h) * (d2.double() * s)[:, :, None, None]
    h = F.relu(F.max_pool2d(y, 2)).view(-1, 320)
    h = F.relu(net.fc1(h)) * (d1.double() * s)
    out = F.log_softmax(net.fc2(h), dim=1)
    loss = F.nll_loss(out, torch.tensor([label]))
    net.zero_grad()
    loss.backward()
    g = torch.cat([p_.grad.flatten() for p_ in (net.conv1.weight, net.conv1.bias, net.conv2.weight, net.conv2.bias)])
    return out[0].detach(), float(loss.detach()), g


@pytest.mark.parametrize("drop", [False, True], ids=["nodrop", "drop"])
def test_fp32_oracle_equals_torch_autograd(drop):
    """dt = fp32 rounds nothing: loss, log-probs and the per-sample conv gradient equal Net().double()
    under autograd to 1e-12 (relative to the tensor's largest magnitude), on synthetic samples and the
    three edge images, with and without the host Philox keep masks."""
    data, net = orc.dataset(), _net64()
    m2, m1 = orc.host_masks(orc.DROP_SEED, 0, 0, 16, 0.5)
    n = len(data)
    for k, i in enumerate([0, 1, 2, 3, 4, n - 3, n - 2, n - 1]):
        kw = dict(keep2=m2[k], keep1=m1[k], drop_p=0.5) if drop else {}
        r = orc.run(data.images[i], int(data.labels[i]), orc.master_params(), FP32, grad_scale=1.0, **kw)
        logp, loss, g = _torch_sample(net, orc.normalise(data.images[i]), int(data.labels[i]),
                                      *((m2[k], m1[k], 0.5) if drop else ()))
        assert abs(r.loss - loss) < 1e-12 * max(1.0, loss)
        assert float((r.logp - logp).abs().max()) < 1e-12 * float(logp.abs().max())
        for name, a, b in CONV_SEGMENTS:
            assert float((r.grad[a:b] - g[a:b]).abs().max()) <= 1e-12 * max(float(g[a:b].abs().max()), 1e-30), (i, name)


def test_pooling_ties_follow_torch():
    """All-zero and all-255 images: every conv1 and conv2 pooling window is a tie between identical
    operand rows; the oracle's argmax is the first position and its pooling backward equals torch's."""
    data, net = orc.dataset(), _net64()
    n = len(data)
    for i in (n - 3, n - 2):
        r = orc.run(data.images[i], int(data.labels[i]), orc.master_params(), FP32)
        assert not bool(r.idx1.any()) and not bool(r.idx2.any())
        _, _, g = _torch_sample(net, orc.normalise(data.images[i]), int(data.labels[i]))
        assert float(g.abs().max()) > 0
        assert float((r.grad - g).abs().max()) <= 1e-12 * float(g.abs().max())
        for dt in (BF16, FP16):
            r16 = orc.run(data.images[i], int(data.labels[i]), orc.master_params(), dt)
            assert not bool(r16.idx1.any()) and not bool(r16.idx2.any())


@pytest.mark.parametrize("dt", [BF16, FP16, FP32], ids=_dt)
def test_pinned_share_and_rounding_band(dt):
    """At least half of the candidates are pinned (a condition on the oracle alone), and the rounding
    band E per conv parameter tensor over them: printed, and positive for the 16-bit types."""
    n = len(orc.dataset())
    pins = orc.pinned_candidates(dt)
    print(f"{_dt(dt)}: {len(pins)} of {n} candidates pinned: {pins}")
    assert 2 * len(pins) >= n
    # the issue's literal rule (no window or ReLU exempt): what the two relaxations in the oracle's
    # docstring buy.  Measured: 30 / 22 / 34 of 48 (bf16 / fp16 / fp32) against 32 / 27 / 42.
    literal = [i for i in range(n) if orc.candidate(dt, i).pinned_literal]
    print(f"{_dt(dt)}: {len(literal)} of {n} pinned under the literal rule: {literal}")
    assert set(literal) <= set(pins)
    # the GPU tests' short tiles and eval batch hold the pinned edge images: the bright pixel for every
    # dtype and at least one of all zero / all 255
    assert n - 1 in pins and len([i for i in pins if i >= n - 3]) >= 2
    risk = max(orc.candidate(dt, i).n_at_risk for i in range(n))
    print(f"{_dt(dt)}: at most {risk} inputs of a sample within theta of a rounding midpoint")
    for dropout in (False, True):
        E = orc.band(dt, dropout)
        print(f"{_dt(dt)}: E{' (dropout)' if dropout else ''} = " + ", ".join(f"{k} {v:.3e}" for k, v in E.items()))
        for name, v in E.items():
            assert (v == 0.0) if dt == FP32 else (0.0 < v < 0.05), (name, v)


def test_bounds_are_positive_and_small():
    """The propagated bounds are finite, non-negative and far below the values they bound."""
    r = orc.candidate(BF16, orc.pinned_candidates(BF16)[0])
    for name in ("p2", "h", "dz1", "dlog", "logp"):
        th = getattr(r, "th_" + name)
        assert bool(torch.isfinite(th).all()) and bool((th >= 0).all()) and float(th.max()) < 1e-2, name
    assert 0 < r.th_loss < 1e-2
    for name, (s, k) in r.dots.items():
        assert k in (25, 250, 320, 50) and bool((s >= 0).all()), name
