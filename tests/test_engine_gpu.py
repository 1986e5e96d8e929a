"""GPU end-to-end: RCCL inside HIP-graph capture, CLIs on the GPU, modular engine training."""
import os
import socket
import subprocess
import sys

import pytest
import torch

from csed_514_project_distributed_training_using_pytorch_amd.data import synthetic_mnist
from csed_514_project_distributed_training_using_pytorch_amd.engine.fused import FusedLeNetTrainer
from csed_514_project_distributed_training_using_pytorch_amd.models import Net

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def test_rccl_allreduce_path_inside_graph_matches_local():
    """World size 1 process group on RCCL: the reduce-only -> all_reduce -> SGD path,
    captured in a HIP graph, must give bit-identical weights to the local path."""
    import torch.distributed as dist

    from csed_514_project_distributed_training_using_pytorch_amd.parallel.comm import init_distributed

    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(_port())
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    if not dist.is_initialized():
        dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev)
    try:
        data = synthetic_mnist(2048, seed=2)
        order = torch.randperm(2048)
        res = []
        for comm in (False, True):
            torch.manual_seed(1)
            eng = FusedLeNetTrainer(Net().to(dev), data, lr=0.02, momentum=0.5, global_batch=64, comm=comm)
            eng.set_epoch_order(order)
            eng.run_steps(20, steps_per_graph=8)
            torch.cuda.synchronize()
            assert eng.capture_comm_ok is True
            res.append(eng.flat.data.clone())
        assert torch.equal(res[0], res[1])
    finally:
        dist.destroy_process_group()


def _run(args, timeout=600):
    env = dict(os.environ)
    env.setdefault("CSED_AUTOBUILD", "0")
    return subprocess.run([sys.executable, *args], cwd=ROOT, capture_output=True, text=True, timeout=timeout,
                          env=env)


@pytest.mark.parametrize("engine", ["fused", "modular"])
def test_train_cli_on_gpu(tmp_path, engine):
    r = _run(["src/train.py", "--synthetic", "--epochs", "2", "--train-size", "19200", "--test-size", "1000",
              "--engine", engine, "--out-dir", str(tmp_path)])
    assert r.returncode == 0, r.stderr[-3000:]
    losses = [float(l.split("Avg. loss: ")[1].split(",")[0]) for l in r.stdout.splitlines() if "Avg. loss" in l]
    # the synthetic set is deliberately hard (86 % after a full 60k epoch on the CPU reference)
    assert len(losses) == 3 and losses[-1] < 0.6 * losses[0], r.stdout[-2000:]
    sd = torch.load(tmp_path / "results" / "model.pth", weights_only=True)
    assert len(sd) == 8 and sd["fc2.bias"].shape == (10,)
    osd = torch.load(tmp_path / "results" / "optimizer.pth", weights_only=True)
    assert len(osd["state"]) == 8 and "momentum_buffer" in osd["state"][0]


def test_train_dist_cli_single_gpu_rank(tmp_path):
    r = _run(["-m", "csed_514_project_distributed_training_using_pytorch_amd.parallel.launch", "--nproc", "1",
              "src/train_dist.py", "--synthetic", "--epochs", "2", "--train-size", "6400", "--test-size", "1000",
              "--out-dir", str(tmp_path)])
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("Epoch=")]
    assert len(lines) == 2
    assert (tmp_path / "model.pt").exists()


def test_bench_contract_json():
    """bench.py prints exactly one JSON line with the driver's fields (short run)."""
    import json

    r = _run(["bench.py", "--steps", "40", "--warmup", "8", "--steps-per-graph", "8", "--no-epoch"])
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.strip().startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    rec = json.loads(lines[0])
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
              "vs_baseline", "dtype", "data", "config"):
        assert k in rec, k
    assert rec["n_gpus"] == 1 and rec["steps"] == 40 and rec["warmup"] == 8 and rec["dtype"] == "bf16"
    assert rec["config"]["global_batch"] == 64 and rec["value"] > 0 and rec["higher_is_better"] is True
    assert abs(rec["value"] - 64 / (rec["ms_per_step"] * 1e-3)) / rec["value"] < 0.01


def test_bench_plain_run_dumps_outputs_and_skips_full_parts(tmp_path):
    """A plain run times the steps only (the --full fields are null) and --dump-outputs writes the
    training state the timed steps left: float32 params / momentum, float64 loss sums."""
    import json

    import numpy as np

    r = _run(["bench.py", "--gpus", "1", "--steps", "24", "--warmup", "4", "--steps-per-graph", "8",
              "--dump-outputs", str(tmp_path / "out")])
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.strip().startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    rec = json.loads(lines[0])
    assert rec["steps"] == 24 and rec["value"] > 0 and rec["ms_per_step"] > 0 and rec["dtype"] == "bf16"
    for k in ("time_elapsed_s", "epoch0_s", "epoch_s", "epoch0_breakdown", "epoch_breakdown"):
        assert rec[k] is None, (k, rec[k])
    assert "fp32" not in rec and "val_acc" not in rec
    out = {p.stem: np.load(p) for p in (tmp_path / "out").iterdir()}
    assert set(out) == {"params", "momentum", "loss"}
    assert out["params"].dtype == np.float32 and out["params"].shape == (21840,)
    assert out["momentum"].dtype == np.float32 and out["momentum"].shape == (21840,)
    assert out["loss"].dtype == np.float64 and out["loss"].shape == (2,)
    assert np.isfinite(out["params"]).all() and np.isfinite(out["momentum"]).all()
    assert np.abs(out["momentum"]).max() > 0  # the steps ran
    # the loss sums cover exactly the 24 timed steps of 64 samples: the line's mean loss (4 decimals),
    # below a uniform guess's ln(10) after the warm-up's training
    assert 0 <= out["loss"][1] <= 24 * 64
    assert abs(out["loss"][0] / (24 * 64) - rec["train_loss_timed_rank0"]) < 1e-4
    assert 0 < out["loss"][0] / (24 * 64) < 2.3026


def test_bench_full_run_reports_epochs_and_fp32():
    """--full keeps what a plain run leaves out: epoch 0 and the reference's span, the warm epoch
    with its validation, and the exact-fp32 sub-record."""
    import json

    r = _run(["bench.py", "--gpus", "1", "--steps", "20", "--warmup", "5", "--full"])
    assert r.returncode == 0, r.stderr[-3000:]
    rec = json.loads([l for l in r.stdout.splitlines() if l.strip().startswith("{")][-1])
    assert rec["value"] > 0 and 0 < rec["time_elapsed_s"] < rec["process_elapsed_s"]
    assert rec["epoch0_s"] > 0 and rec["epoch_s"] > 0 and 0 <= rec["val_acc"] <= 1
    assert rec["epoch0_breakdown"]["replays"] > 0 and rec["epoch_breakdown"]["replays"] > 0
    assert rec["fp32"]["value"] > 0 and rec["fp32"]["epoch_s"] > 0


def test_graft_smoke_entry():
    r = _run(["-c", "import __graft_entry__ as g; g.smoke()"])
    assert r.returncode == 0, r.stderr[-3000:]
    assert "smoke ok" in r.stdout

