"""Time the fused engine's graph-replayed step under SGD and under Adam (FusedLeNetTrainer(optimizer="adam")):
500 replayed steps at global batch 64, bf16 and fp32, alternating sgd / adam, the median of each.  Prints one
JSON line.  profiles/adam.md records a run."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from csed_514_project_distributed_training_using_pytorch_amd.data.mnist import synthetic_mnist  # noqa: E402
from csed_514_project_distributed_training_using_pytorch_amd.engine.fused import FusedLeNetTrainer  # noqa: E402
from csed_514_project_distributed_training_using_pytorch_amd.models import Net  # noqa: E402


def main() -> int:
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--steps", type=int, default=500)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--global-batch", type=int, default=64)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    n = args.global_batch * (args.steps + args.warmup)
    order = torch.arange(n) % 4096
    data = synthetic_mnist(4096, seed=3)
    out = {"steps": args.steps, "global_batch": args.global_batch}
    for name, dtype in (("bf16", torch.bfloat16), ("fp32", torch.float32)):
        engines = {}
        for kind in ("sgd", "adam"):
            torch.manual_seed(1)
            engines[kind] = FusedLeNetTrainer(Net().to(dev), data, lr=0.01 if kind == "sgd" else 0.001,
                                              global_batch=args.global_batch, compute_dtype=dtype, optimizer=kind)
        times = {"sgd": [], "adam": []}
        for _ in range(args.rounds):
            for kind, eng in engines.items():
                eng.set_epoch_order(order)
                plan = eng.step_plan(args.steps, 32)  # (captured here, outside the timed region)
                eng.run_steps(args.warmup, 32)
                torch.cuda.synchronize(dev)
                t0 = time.perf_counter()
                for launch in plan:
                    launch()
                torch.cuda.synchronize(dev)
                times[kind].append(1e6 * (time.perf_counter() - t0) / args.steps)
        out[name] = {k: {"median_us_per_step": round(statistics.median(v), 3), "runs_us": [round(x, 3) for x in v]}
                     for k, v in times.items()}
        for eng in engines.values():
            eng.close()
    print(json.dumps(out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
