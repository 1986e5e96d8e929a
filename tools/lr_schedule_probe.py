"""Cost of the device-resident learning-rate schedule in the fused step: us/step of K graph-replayed steps
with and without an optim.LRSchedule, at global batch 64 and 8 (one GPU).

With a table lenet_update runs its SCHED instantiation: two more loads per block (position, table entry) and,
at the block's tail, the ticket (a __syncthreads and one atomic) that lets the last block advance the position.
Runs alternate (plain, scheduled, plain, ...) so that drift hits both alike; the median of each is printed as
one JSON line per batch size.

    python tools/lr_schedule_probe.py [--steps 900] [--repeats 5] [--batches 64 8]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from csed_514_project_distributed_training_using_pytorch_amd.data import synthetic_mnist  # noqa: E402
from csed_514_project_distributed_training_using_pytorch_amd.engine.fused import FusedLeNetTrainer  # noqa: E402
from csed_514_project_distributed_training_using_pytorch_amd.models import Net  # noqa: E402
from csed_514_project_distributed_training_using_pytorch_amd.optim import LRSchedule  # noqa: E402


def _engine(batch: int, n: int, scheduled: bool, steps: int) -> FusedLeNetTrainer:
    torch.manual_seed(1)
    dev = torch.device("cuda", 0)
    eng = FusedLeNetTrainer(Net().to(dev), synthetic_mnist(n, seed=0), lr=0.01, momentum=0.5, global_batch=batch)
    if scheduled:
        eng.set_lr_schedule(LRSchedule.warmup_cosine(0.01, min(100, steps // 2), max(2, steps)))
    eng.set_epoch_order(torch.randperm(n, generator=torch.Generator().manual_seed(0)))
    return eng


def _time(eng: FusedLeNetTrainer, steps: int) -> float:
    """us/step of ``steps`` graph-replayed steps (graphs resolved before the clock starts)."""
    eng.cursor.zero_()
    plan = eng.step_plan(steps)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for launch in plan:
        launch()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e6 / steps


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--steps", type=int, default=900)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--batches", type=int, nargs="+", default=[64, 8])
    args = ap.parse_args(argv)
    for batch in args.batches:
        n = batch * args.steps
        engines = {"plain": _engine(batch, n, False, args.steps), "scheduled": _engine(batch, n, True, args.steps)}
        for eng in engines.values():  # capture + one untimed pass
            _time(eng, args.steps)
        runs = {k: [] for k in engines}
        for _ in range(args.repeats):
            for k, eng in engines.items():
                runs[k].append(_time(eng, args.steps))
        med = {k: statistics.median(v) for k, v in runs.items()}
        print(json.dumps({"global_batch": batch, "steps": args.steps, "repeats": args.repeats,
                          "plain_us_per_step": round(med["plain"], 3),
                          "scheduled_us_per_step": round(med["scheduled"], 3),
                          "delta_us": round(med["scheduled"] - med["plain"], 3),
                          "plain_runs": [round(v, 3) for v in runs["plain"]],
                          "scheduled_runs": [round(v, 3) for v in runs["scheduled"]]}), flush=True)
        for eng in engines.values():
            eng.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
