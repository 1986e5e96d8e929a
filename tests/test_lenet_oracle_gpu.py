"""csed::lenet_train, lenet_tile and lenet_train_f32 (and the eval kernels) per sample against the fp64
oracle of one sample (tests/_lenet_oracle.py; tests/test_lenet_oracle_cpu.py ties that oracle to torch
autograd and asserts the pinned share).  Every launch goes through eng.train_args(...) and the slab, the
vector slab and the loss partials are read directly: no lenet_update in between, nothing is diluted by a
batch sum.  Only *pinned* samples are compared (pool / ReLU decisions provably not at risk: the kernel's
backward is then the oracle's linear map), 16-bit gradients against the rounding-matched oracle.

Bounds.  P2, H, dZ1, dlogits per element: the oracle's propagated theta + 1/2 ulp(dt), against its
unrounded value.  Loss, log-probs: the bound derived in the oracle's docstring.  Conv gradient, relative
L2 per parameter tensor and slab row: E / 2 for bf16 / fp16, E the rounding band (largest distance over
the pinned candidates between the oracle with the backward's rounding points on and off: what one layer
of 16-bit rounding is worth -- a kernel that rounds where the oracle rounds sits clearly nearer).  For
fp32 the effective bound is the flat 1e-4 the suite already holds that kernel to: the propagated
(K + 2) 2^-24 bound is computed and the smaller of the two is taken, but the propagated one is a worst case
through sums that cancel (0.05 for conv2, about 1 for conv1, relative L2) and is never the smaller.

What bites and what does not.  The conv-gradient check is the sharp one.  The propagated thetas of P2, H,
dZ1, dlogits, the log-probs and the loss are worst-case bounds too (up to about 2e-4, 9e-4, 3e-4 and, for
the loss, 2e-2 on a bf16 sample, against observed errors near 1e-7): derived, not fitted, and they catch
gross errors only -- a dropped mask, a wrong unit, a missing scale.  The 16-bit gradient check's sensitivity
is E / 2, about 10^4 times the bf16 kernel's actual distance: a scratch build that drops ONE pixel from the
split step's conv1-wgrad sum fails it narrowly for bf16 (2.8e-3 against 2.6e-3) and clearly for fp16
(4.3e-3 against 3.6e-4).

E (computed on the CPU, tests/test_lenet_oracle_cpu.py prints it) and the kernels' largest measured
distance over all groups of this file (MI355X, 2026-10-19):

                      conv1.weight  conv1.bias  conv2.weight  conv2.bias
    bf16  E                5.124e-03   5.585e-03    3.330e-03   3.748e-03
          E, dropout       4.225e-03   7.074e-03    4.231e-03   7.795e-03
          measured         2.538e-07   3.388e-08    4.189e-08   0
    fp16  E                7.166e-04   7.166e-04    5.409e-04   5.537e-04
          E, dropout       7.266e-04   9.663e-04    5.288e-04   1.118e-03
          measured         3.169e-05   5.347e-05    1.343e-05   0
    fp32  measured         1.614e-06   1.334e-06    7.536e-07   4.612e-07

(bf16 sits at fp32 summation noise: the kernel rounds exactly where the oracle does.  fp16's distance is
a few dZ1 / gradient-image elements landing on the other side of a rounding midpoint.)  The whole file
takes about 4 s on the GPU.
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _lenet_oracle as orc  # noqa: E402
from _lenet_oracle import BF16, CONV_SEGMENTS, DROP_SEED, FP16, FP32, U  # noqa: E402
from _update_oracle import (N_DLOG, N_DZ1, N_H, N_P2, O_C2W, SLOT_OF_PARAM, SPLIT_K, V_DLOG, V_DZ1, V_H, V_P2, VEC,  # noqa: E402
                            slab_off)

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda", 0)
DTYPES = [BF16, FP16, FP32]
MEASURED: dict = {}  # (dtype, tensor) -> largest relative-L2 distance seen (printed; see the header)


def _dt(dtype) -> str:
    return str(dtype).replace("torch.", "")


def _order(dt, n_pinned: int, edges: bool = True) -> list[int]:
    """The first ``n_pinned`` pinned candidates of dt (+ the three edge images)."""
    n = len(orc.dataset())
    pins = [i for i in orc.pinned_candidates(dt) if i < n - 3][:n_pinned]
    assert len(pins) == n_pinned
    return pins + ([n - 3, n - 2, n - 1] if edges else [])


def _order_all_pinned(dt, B: int) -> list[int]:
    """B candidates that are ALL pinned for dt: the first pinned synthetic ones, then -- last, so that they
    fall into a short last tile -- the edge images that are pinned for dt (the bright pixel for every
    dtype; all zero for fp16 and fp32, all 255 for bf16 and fp32)."""
    n = len(orc.dataset())
    pins = orc.pinned_candidates(dt)
    edge = [i for i in pins if i >= n - 3]
    assert n - 1 in edge and len(edge) >= 2
    order = [i for i in pins if i < n - 3][:B - len(edge)] + edge
    assert len(order) == B
    return order


def _engine(dt, order, drop_p=0.0, **kw):
    from csed_514_project_distributed_training_using_pytorch_amd.engine.fused import FusedLeNetTrainer
    from csed_514_project_distributed_training_using_pytorch_amd.models import Net

    torch.manual_seed(orc.WEIGHT_SEED)
    eng = FusedLeNetTrainer(Net().to(DEV), orc.dataset(), global_batch=len(order), compute_dtype=dt, drop_p=drop_p,
                            seed=DROP_SEED, **kw)
    assert torch.equal(eng.flat.data.cpu(), orc.master_params())
    eng.set_epoch_order(torch.tensor(order))
    return eng


def _launch(eng, **kw):
    """One lenet_train launch into a NaN-filled slab and loss partials; returns its TrainArgs."""
    eng.slab.fill_(float("nan"))
    eng.loss_parts.fill_(float("nan"))
    args = eng.train_args(**kw)
    torch.ops.csed.lenet_train(*args)
    torch.cuda.synchronize()
    return args


def _slab_rows(eng, G: int, B: int):
    """(conv1 [G, 260], conv2 [min(G, B), 5020]) of the slab, in flat parameter order, fp64."""
    flat = eng.slab.view(-1).cpu().double().numpy()
    R2 = min(G, B)
    c1 = flat[slab_off(SLOT_OF_PARAM[None, :O_C2W], np.arange(G)[:, None], G, R2)]
    c2 = flat[slab_off(SLOT_OF_PARAM[None, O_C2W:], np.arange(R2)[:, None], G, R2)]
    return torch.from_numpy(c1), torch.from_numpy(c2)


def _half_ulp(v, th, dt):
    return orc.ulp(v.abs() + th, dt) / 2


def _check_vectors(eng, dt, res, what):
    """P2, H, dZ1, dlogits of every pinned sample within theta + 1/2 ulp(dt) of the oracle's unrounded
    values; the features the layout says are never written are zero."""
    v = eng.fc_vectors(len(res)).cpu().double()
    written = torch.zeros(VEC, dtype=torch.bool)
    for off, n, name in ((V_P2, N_P2, "p2"), (V_DZ1, N_DZ1, "dz1"), (V_H, N_H, "h"), (V_DLOG, N_DLOG, "dlog")):
        written[off:off + n] = True
        for b, r in enumerate(res):
            if not r.pinned:
                continue
            want, th = getattr(r, name), getattr(r, "th_" + name)
            bound = th + _half_ulp(want, th, dt)
            err = (v[b, off:off + n] - want).abs()
            bad = ~(err <= bound)
            if bad.any():
                i = int(torch.nonzero(bad)[0])
                raise AssertionError(f"{what}: {name}[{i}] of sample {b}: got {v[b, off + i].item()!r}, want "
                                     f"{want[i].item()!r}, bound {bound[i].item():.3e}; worst error / bound "
                                     f"{(err / bound.clamp_min(1e-300)).max().item():.3f}")
    assert not bool(v[:, ~written].any()), f"{what}: a feature the layout never writes is not zero"


def _check_loss(eng, res, groups, G, what):
    """Loss partials per workgroup: ``groups[g]`` = the batch positions workgroup g reports (none: zero)."""
    lp = eng.loss_parts[:2 * G].cpu().double().view(G, 2)
    for g in range(G):
        rs = [res[b] for b in groups.get(g, [])]
        if not rs:
            assert lp[g].tolist() == [0.0, 0.0], f"{what}: workgroup {g} reports no sample but wrote {lp[g].tolist()}"
            continue
        if not all(r.pinned for r in rs):
            continue
        want = sum(r.loss for r in rs)
        bound = sum(r.th_loss for r in rs) + len(rs) * U * sum(abs(r.loss) for r in rs)
        print(f"{what}: workgroup {g} loss error {abs(lp[g, 0].item() - want):.3e} bound {bound:.3e}")
        assert abs(lp[g, 0].item() - want) <= bound, f"{what}: workgroup {g} loss {lp[g, 0].item()!r}, want {want!r}, bound {bound:.3e}"
        if all(r.pred_safe for r in rs):
            assert lp[g, 1].item() == sum(r.correct for r in rs), f"{what}: workgroup {g} correct count"


def _check_rows(dt, got, lo_hi, res, members, dropout, what):
    """Slab rows ``got`` [rows, n] (parameters lo_hi[0] .. lo_hi[1] of the flat order) against the sum of
    the oracle gradients of ``members[row]`` (batch positions), per parameter tensor inside the range."""
    E = orc.band(dt, dropout) if dt != FP32 else None
    for row, pos in members.items():
        rs = [res[b] for b in pos]
        if not all(r.pinned for r in rs):
            continue
        for name, a, b in CONV_SEGMENTS:
            if a < lo_hi[0] or b > lo_hi[1]:
                continue
            g = got[row, a - lo_hi[0]:b - lo_hi[0]]
            want = sum(r.grad[a:b] for r in rs)
            if float(want.norm()) == 0.0:
                assert not bool(g.any()), f"{what}: {name} row {row}: the oracle gradient is exactly zero, the kernel's is not"
                continue
            dist = orc.rel_l2(g, want)
            if dt == FP32:
                err = sum(r.grad_err[a:b] for r in rs) + len(rs) * U * sum(r.grad[a:b].abs() for r in rs)
                bound = min(float(err.norm() / want.norm()), 1e-4)
            else:
                bound = E[name] / 2
            key = (_dt(dt), name)
            MEASURED[key] = max(MEASURED.get(key, 0.0), dist)
            assert dist <= bound, (f"{what}: {name} row {row} (batch positions {pos}): relative L2 {dist:.3e} to the "
                                   f"rounding-matched oracle, bound {bound:.3e}")


def _check(eng, dt, order, args, conv1_members, conv2_members, loss_groups, what, drop_key=None, all_pinned=False):
    """All assertions of one training launch.  ``conv1_members``: {tuple of slab rows summed: batch positions},
    ``conv2_members``: {slab row: batch positions}, ``drop_key``: (counter, rank) of a dropout launch.
    ``all_pinned``: every sample must be pinned, so that no slab row or loss partial is left uncompared
    (a row with an unpinned member is skipped; where rows hold several samples that must not happen)."""
    B, G = args.B, args.grid
    res = [orc.candidate(dt, i, None if drop_key is None else (*drop_key, B, b), float(args.grad_scale))
           for b, i in enumerate(order)]
    npin = sum(r.pinned for r in res)
    assert npin >= B // 2, f"{what}: only {npin} of {B} samples pinned"
    assert npin == B or not all_pinned, f"{what}: samples {[b for b, r in enumerate(res) if not r.pinned]} are not pinned"
    _check_vectors(eng, dt, res, what)
    _check_loss(eng, res, loss_groups, G, what)
    c1, c2 = _slab_rows(eng, G, B)
    c1sum = torch.stack([c1[list(rows)].sum(0) for rows in conv1_members])
    _check_rows(dt, c1sum, (0, O_C2W), res, dict(enumerate(conv1_members.values())), drop_key is not None, what + " conv1")
    _check_rows(dt, c2, (O_C2W, orc.CNP), res, conv2_members, drop_key is not None, what + " conv2")
    print(f"{what}: {npin}/{B} pinned; measured so far", {k: f"{v:.3e}" for k, v in MEASURED.items() if k[0] == _dt(dt)})


def _per_sample(B):
    return {(b,): [b] for b in range(B)}, {b: [b] for b in range(B)}, {b: [b] for b in range(B)}


# ------------------------------------------------------------------ (a) one workgroup per sample, (e) dropout keys
@pytest.mark.parametrize("drop_p", [0.0, 0.5], ids=["nodrop", "drop"])
@pytest.mark.parametrize("dt", DTYPES, ids=_dt)
def test_one_workgroup_per_sample(dt, drop_p):
    """B = 16 (13 pinned candidates + all zero, all 255, one bright pixel at (27, 27)), split=False: a
    slab row is the sample's conv gradient.  Staged and staged=False.  With dropout (keep masks from the
    host Philox reference): Philox offsets 0 and 3, and rank 1 (mask element index rank * B + position)."""
    order = _order(dt, 13)
    assert orc.candidate(dt, order[-1]).pinned, "the bright-pixel image must be among the compared samples"
    eng = _engine(dt, order, drop_p=drop_p, split=False)
    assert eng.grid == 16 and not eng.split
    m1, m2, lg = _per_sample(16)
    runs = [(0, 0, {}), (0, 0, dict(staged=False))] if drop_p == 0 else \
        [(0, 0, {}), (0, 0, dict(staged=False)), (3, 0, {}), (0, 1, dict(rank=1, staged=False))]
    for counter, rank, kw in runs:
        eng.rng_offset.fill_(counter)
        args = _launch(eng, **kw)
        _check(eng, dt, order, args, m1, m2, lg, f"{_dt(dt)} B 16 drop {drop_p} counter {counter} rank {rank} {kw}",
               drop_key=(counter, rank) if drop_p else None)


# ------------------------------------------------------------------ (b) split step
@pytest.mark.parametrize("dt", DTYPES, ids=_dt)
def test_split_step(dt):
    """B = 8 on 32 workgroups: conv2 rows per sample, a sample's four conv1 partial rows (workgroups b,
    b + 8, b + 16, b + 24) sum to its conv1 gradient, part 0 alone wrote the vectors and the loss."""
    order = _order(dt, 5)
    eng = _engine(dt, order)
    assert eng.split and eng.grid == SPLIT_K * 8
    args = _launch(eng)
    m1 = {tuple(b + 8 * k for k in range(SPLIT_K)): [b] for b in range(8)}
    _check(eng, dt, order, args, m1, {b: [b] for b in range(8)}, {b: [b] for b in range(8)}, f"{_dt(dt)} split B 8")


# ------------------------------------------------------------------ (c) several samples per workgroup
@pytest.mark.parametrize("dt", DTYPES, ids=_dt)
def test_sample_pipeline(dt):
    """B = 13 on 5 workgroups (3, 3, 3, 2, 2 samples through the sample pipeline), every sample pinned: a
    row is the sum of its samples' gradients (workgroup g: samples g, g + 5, g + 10)."""
    order = _order(dt, 13, edges=False)
    eng = _engine(dt, order, grid=5)
    assert eng.grid == 5 and not eng.staged
    args = _launch(eng)
    mem = {g: list(range(g, 13, 5)) for g in range(5)}
    assert all(orc.candidate(dt, i, None, float(args.grad_scale)).pinned for i in order)
    _check(eng, dt, order, args, {(g,): p for g, p in mem.items()}, mem, mem, f"{_dt(dt)} B 13 grid 5", all_pinned=True)


# ------------------------------------------------------------------ (d) tile kernel
@pytest.mark.parametrize("B", [7, 9])
@pytest.mark.parametrize("dt", [BF16, FP16], ids=_dt)
def test_tile_kernel(dt, B):
    """train_kernel = 2: tiles of 4 samples, a short last tile of 3 (B = 7) and of 1 (B = 9); workgroup g
    holds tile g.  Every sample is pinned, the short tile's included (it holds the pinned edge images), so
    every row and every loss partial is compared."""
    order = _order_all_pinned(dt, B)
    G = (B + 3) // 4
    eng = _engine(dt, order, grid=G)
    eng.train_kernel = 2
    assert eng.uses_tile_kernel(B, G)
    args = _launch(eng)
    assert args.kernel == 2
    mem = {g: list(range(4 * g, min(4 * g + 4, B))) for g in range(G)}
    _check(eng, dt, order, args, {(g,): p for g, p in mem.items()}, mem, mem, f"{_dt(dt)} tile B {B}", all_pinned=True)


# ------------------------------------------------------------------ (f) evaluation
@pytest.mark.parametrize("dt,kernel", [(BF16, 1), (BF16, 2), (FP16, 1), (FP16, 2), (FP32, 0)],
                         ids=lambda v: _dt(v) if isinstance(v, torch.dtype) else f"k{v}")
def test_eval_log_probs(dt, kernel):
    """lenet_eval on 5 samples, all pinned (the pinned edge images among them): the per-sample log-probs
    within the oracle's bound (logit theta + the softmax's fp32 terms), the loss / correct partials."""
    from csed_514_project_distributed_training_using_pytorch_amd.data.mnist import MNIST_MEAN, MNIST_STD, MNISTData

    order = _order_all_pinned(dt, 5)
    eng = _engine(dt, order)
    d = orc.dataset()
    test = MNISTData(d.images[order], d.labels[order], True).to(DEV)
    out = torch.full((5, 10), float("nan"), device=DEV)
    parts = torch.full((512,), float("nan"), device=DEV)
    torch.ops.csed.lenet_eval(test.images, test.labels, torch.arange(5, device=DEV), 5, eng.wimg, eng.flat.data,
                              MNIST_MEAN, MNIST_STD, parts, out, eng.mfma, kernel)
    torch.cuda.synchronize()
    res = [orc.candidate(dt, i) for i in order]
    assert all(r.pinned for r in res)
    for b, r in enumerate(res):
        err = (out[b].cpu().double() - r.logp).abs()
        assert bool((err <= r.th_logp).all()), f"sample {b}: log-prob error / bound {(err / r.th_logp).max().item():.3f}"
    G = 5 if kernel != 2 else 2
    lp = parts[:2 * G].cpu().double().view(G, 2).sum(0)
    assert abs(lp[0].item() - sum(r.loss for r in res)) <= sum(r.th_loss for r in res) + 5 * U * sum(r.loss for r in res)
    if all(r.pred_safe for r in res):
        assert lp[1].item() == sum(r.correct for r in res)
