"""Measure the per-epoch affine augmentation (data.AffineAugment, csrc/kernels/augment.hip) on the synthetic set:
the kernel's time for the whole 60,000-row epoch order and for a 7,500-row shard (device events around back-to-back
launches, so launch gaps are included: an upper bound), the fused engine's warm epoch time with and without
--augment-shift 2 --augment-rotate 15 (two engines, alternating), and validation accuracy after 3 epochs with and
without.  --elastic ALPHA SIGMA measures data.ElasticAugment (csrc/kernels/augment_elastic.hip) on top of the same
affine maxima instead: its launches next to the affine kernel's in the same run, and "on" is the elastic augmenter.
--stroke T P measures data.StrokeAugment (csrc/kernels/augment_stroke.hip): its own launch next to the affine
kernel's, and "on" is the stroke augmenter alone or, under --shift PX, around an AffineAugment of that shift.
Prints one JSON line.  profiles/augment.md records a run."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from csed_514_project_distributed_training_using_pytorch_amd.data import AffineAugment, ElasticAugment, StrokeAugment, synthetic_mnist  # noqa: E402
from csed_514_project_distributed_training_using_pytorch_amd.engine.fused import FusedLeNetTrainer  # noqa: E402
from csed_514_project_distributed_training_using_pytorch_amd.models import Net  # noqa: E402


def kernel_us(aug, src, dst, idx, launches: int, rounds: int) -> list[float]:
    out = []
    for _ in range(rounds + 1):  # (the first round is the warm-up)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(launches):
            aug.apply(src, dst, idx=idx)
        b.record()
        b.synchronize()
        out.append(1e3 * a.elapsed_time(b) / launches)
    return [round(v, 3) for v in out[1:]]


def engine(dev, train, aug):
    torch.manual_seed(1)
    eng = FusedLeNetTrainer(Net().to(dev), train, global_batch=64, compute_dtype=torch.bfloat16)
    eng.set_augment(aug)
    return eng


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--train-size", type=int, default=60000)
    ap.add_argument("--test-size", type=int, default=10000)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--elastic", type=float, nargs=2, default=None, metavar=("ALPHA", "SIGMA"))
    ap.add_argument("--stroke", type=float, nargs=2, default=None, metavar=("T", "P"))
    ap.add_argument("--erase-size", type=int, nargs=2, default=[4, 12], metavar=("LO", "HI"))
    ap.add_argument("--shift", type=float, default=0.0, metavar="PX", help="with --stroke: the inner augmenter's shift")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    train, test = synthetic_mnist(args.train_size, seed=0), synthetic_mnist(args.test_size, seed=0, train=False)
    n = len(train)
    affine = lambda: AffineAugment(max_shift=2, max_rot_deg=15, seed=1)  # noqa: E731
    make = affine if args.elastic is None else lambda: ElasticAugment(*args.elastic, max_shift=2, max_rot_deg=15, seed=1)
    stroke = None
    if args.stroke is not None:  # the stroke kernel alone is what is timed; "on" may wrap an affine augmenter
        stroke = lambda inner=None: StrokeAugment(*args.stroke, tuple(args.erase_size), inner=inner, seed=1)  # noqa: E731
        make = lambda: stroke(AffineAugment(max_shift=args.shift, seed=1) if args.shift else None)  # noqa: E731
    src = train.images.to(dev)
    dst = src.clone()
    gen = torch.Generator().manual_seed(0)
    order = torch.randperm(n, generator=gen).to(dev)
    rec = {"rows": n, "kernel_us": {str(m): kernel_us((stroke or make)(), src, dst, order[:m].contiguous(), 50, args.rounds)
                                    for m in (n, n // 8)}}
    if args.elastic is not None or stroke is not None:  # the affine kernel's figure from the same run, to set it against
        rec.update({"elastic": args.elastic} if stroke is None else {"stroke": args.stroke, "shift": args.shift})
        rec["affine_kernel_us"] = {str(m): kernel_us(affine(), src, dst, order[:m].contiguous(), 50, args.rounds)
                                   for m in (n, n // 8)}
    engs = {"off": engine(dev, train, None), "on": engine(dev, train, make())}
    epoch_ms = {"off": [], "on": []}
    for r in range(args.rounds + 1):  # (round 0 captures the graphs and warms up)
        host_order = torch.randperm(n, generator=gen)
        for kind, eng in engs.items():
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            eng.train_epoch(host_order)
            torch.cuda.synchronize(dev)
            if r:
                epoch_ms[kind].append(round(1e3 * (time.perf_counter() - t0), 3))
    rec["warm_epoch_ms"] = {k: {"median": statistics.median(v), "runs": v} for k, v in epoch_ms.items()}
    for eng in engs.values():
        eng.close()
    acc = {}
    for kind, aug in (("off", None), ("on", make())):
        eng = engine(dev, train, aug)
        g = torch.Generator().manual_seed(5)
        for _ in range(3):
            eng.train_epoch(torch.randperm(n, generator=g))
        loss, correct = eng.evaluate(test)
        acc[kind] = {"val_loss": round(loss / len(test), 4), "accuracy": round(100.0 * correct / len(test), 2)}
        eng.close()
    rec["after_3_epochs"] = acc
    print(json.dumps(rec))
    return 0


if __name__ == "__main__":
    sys.exit(main())
