"""Bring-up of the fused engine's gradient exchange: plain functions on a ``FusedLeNetTrainer``.

The data-parallel gradient all-reduce is fused into lenet_update (engine/fused.py).  It is enabled after a
collective bring-up and an exact self-test; if either fails, or ``CSED_ALLREDUCE=rccl`` asks for it, the
step runs as the fallback

    lenet_update (reduce only) -> RCCL all-reduce -> SGD kernel

In ``auto`` mode with one rank per GPU (a real node, pushes over xGMI) both steps are then timed at
bring-up -- one 16-step graph each -- and the faster is kept, so a fused exchange slower than RCCL is
never locked in.  ``CSED_TIME_PATHS``: ``auto`` (default: time exactly then), ``1``
(always time, also on ranks sharing a GPU, and also time an exchange-free step), ``0`` (never: a passing
self-test keeps the fused path).

Everything here is collective: every rank runs the same calls in the same order and takes the same
branches."""
from __future__ import annotations

import os
import sys
import time

import torch
import torch.distributed as dist

from ..models.net import N_PARAMS
from ..ops import _native
from ..parallel import comm as _comm
from ..parallel import ipc as _ipc
from .replay import _clear_hip_error, preserved


def enable_exchange(eng, required: bool) -> None:
    """Bring up lenet_update's in-kernel exchange (collective on every rank): open the IPC
    buffers and self-test them with the update kernel itself.  Then (auto mode, RCCL, see
    the module docstring for ``CSED_TIME_PATHS``) the fused and fallback steps are timed
    and the faster is kept."""
    from .fused import lenet_layout

    t0 = time.perf_counter()
    xd = eng._xdiag
    xd["peer_access"] = _ipc.peer_access(eng.device)
    ex, why = _ipc.open_exchange(eng.ctx, lenet_layout().exch_words, shared=eng._xdiag.get("ranks_per_gpu"))
    hook = _ipc.test_reject_hook()
    last = eng.ctx.rank == eng.ctx.world_size - 1
    if hook == "open":  # (test hook: the last rank's mapping "fails"; every rank votes)
        ok_local = not last
        if not vote(eng, ok_local) and ex is not None:
            ex.close()
            ex, why = None, "open: test hook CSED_TEST_EXCH_REJECT=open on the last rank"
    xd["ipc_open"] = "ok" if ex is not None else (why or "failed")
    t1 = time.perf_counter()
    eng.bringup_s["ipc_open"] = t1 - t0
    ok = ex is not None
    if ok:
        eng.exch = ex
        local_ok = exchange_self_test(eng)
        if hook == "selftest" and last:
            local_ok = False
        xd["self_test"] = bool(local_ok)
        ok = vote(eng, local_ok)
        if not ok:
            why = "self-test mismatch or timeout on some rank"
            xd["self_test_all_ranks"] = False
    eng.bringup_s["self_test"] = time.perf_counter() - t1
    if not ok:
        if ex is not None:
            try:
                ex.close()  # collective: every rank opened it (a failed rank's buffer too)
            except Exception:
                pass
        eng.exch = None
        eng.exchange_note = f"fused exchange off: {why}; fallback {eng.allreduce_kind}"
        if required:
            raise RuntimeError(f"CSED_ALLREDUCE=fused but the fused exchange is unusable ({why})")
        return
    eng.exchange_note = "fused exchange on (self-test passed)"
    tp = os.environ.get("CSED_TIME_PATHS", "auto").strip().lower()
    if not required and tp != "0":
        # (every rank takes the same branch: ranks_per_gpu is the group's value).  On gloo
        # (ranks sharing a GPU, a rehearsal) only CSED_TIME_PATHS=1 times: the fallback step's
        # host all-reduce cannot be captured, so it times as inf and the fused path is kept --
        # what the rehearsal measures is the selection's own bring-up cost
        do_time = tp == "1" or (eng.ctx.backend == "nccl" and eng._xdiag.get("ranks_per_gpu") == 1)
    else:
        do_time = False
    if do_time and eng.ctx.control is not None:
        # lazy RCCL (bench.py at N > 1): the fallback step's all-reduce would create the RCCL
        # communicator (1-3.6 s) in the middle of the bring-up -- the selection is deferred to
        # select_path(), which the bench runs after epoch 0 (outside the reference span)
        eng._path_pending = tp
        eng.exchange_note = "fused exchange on (self-test passed; path timing deferred)"
    elif do_time:
        select_path_now(eng, tp)


def select_path_now(eng, tp: str) -> None:
    t2 = time.perf_counter()
    t_fused = time_steps(eng)
    saved, eng.exch = eng.exch, None
    # (gloo: the host all-reduce is not capturable -- not timed, the fused path is kept)
    t_fallback = time_steps(eng) if eng.ctx.backend == "nccl" else float("inf")
    t_local = float("inf")
    if tp == "1":
        # the same step with no exchange at all (each rank updates on its own gradient;
        # the state is restored): fused - local = what the exchange costs per step
        eng.comm = False
        t_local = time_steps(eng)
        eng.comm = True
    # a path whose graph could not be captured times as inf; ties keep the fused path
    eng.exch = saved if t_fused <= t_fallback else None
    if eng.exch is None:
        eng.exchange_note = "fused exchange off: slower than the fallback step"
        # every rank finished the timing above (device synchronize before the timing
        # all-reduce), so no peer still pushes into these buffers: the close is safe
        saved.close()
    else:
        eng.exchange_note = "fused exchange on (self-test passed, timed faster than the fallback)"
    fin = lambda t: round(t, 2) if t != float("inf") else None  # noqa: E731
    eng.path_timing_us = {"fused_step_us": fin(t_fused), "fallback_step_us": fin(t_fallback),
                          "local_step_us": fin(t_local),
                          "exchange_us": fin(t_fused - t_local) if max(t_fused, t_local) != float("inf")
                          else None,
                          "fallback": "rccl", "kept": "fused" if eng.exch is not None else "rccl"}
    eng.bringup_s["path_timing"] = time.perf_counter() - t2


def exchange_diag(eng) -> dict:
    """This rank's data-parallel diagnostics (``parallel/ipc.py`` DIAG_KEYS): the bring-up's
    stage results plus the exchange's current error word and first recorded mismatch."""
    d = _ipc.empty_diag(eng.ctx)
    d.update(eng._xdiag)
    d["device_count"] = torch.cuda.device_count()
    d["path_timing_us"] = eng.path_timing_us
    d["allreduce"] = eng.allreduce_kind
    d["note"] = eng.exchange_note
    if eng.exch is not None:
        d["error_word"] = eng.comm_errors()
        d["first_mismatch"] = eng.comm_diag()
    return d


def vote(eng, ok: bool) -> bool:
    t = torch.tensor([1 if ok else 0], dtype=torch.int32, device=_comm.ctl_device(eng.ctx))
    _comm.ctl_all_reduce(eng.ctx, t, dist.ReduceOp.MIN)
    return bool(t.item())


def exchange_self_test(eng, rounds: int = 2) -> bool:
    """Integer-valued slabs through lenet_update with and without the exchange: the
    exchanged gradient must equal the process group's sum of the local ones exactly
    (both slot parities, every rank).  Runs the same collectives on every rank.  The operands
    come from the extension's own fill kernel (csed::lenet_selftest_fill: small integers, a
    hash of the element index, the round and the rank) and the results are compared on the
    host, so the bring-up launches no torch kernel (each is a code object loaded at its first
    launch, ms apiece -- the round-5 self-test drew its values with torch.randint)."""
    import numpy as np

    ops = torch.ops.csed
    pg_dev = _comm.ctl_device(eng.ctx)
    raw = dict(with_loss=False, grad_scale=1.0)  # (plain slab sums; the local one without the split-K scratch)
    ok = True
    # every round's local and exchanged gradients first, then ONE process-group all-reduce of
    # all the local ones (a collective round trip per round was most of the self-test's time)
    local = torch.empty(rounds, N_PARAMS, dtype=torch.float32, device=eng.device)
    fused = torch.empty_like(local)
    for r in range(rounds):
        ops.lenet_selftest_fill(eng.slab, eng.vslab, eng.B, eng.mfma, 977 + 31 * eng.ctx.rank + 7919 * r)
        ops.lenet_update(*eng.update_args("reduce", grad=local[r], exchange=False, fc_split=False, **raw))
        try:
            ops.lenet_update(*eng.update_args("reduce", grad=fused[r], exchange=True, **raw))
        except Exception:
            ok = False
    ref = local.to(pg_dev, copy=True)
    _comm.ctl_all_reduce(eng.ctx, ref)
    ok &= bool(np.array_equal(fused.cpu().numpy(), ref.cpu().numpy()))
    torch.cuda.synchronize(eng.device)
    try:
        ok &= eng.exch.error(reset=True) == 0
    except Exception:
        ok = False
    _native.zero_(eng.vslab)
    return ok


def time_steps(eng, nsteps: int = 16, reps: int = 3) -> float:
    """us per training step of a captured graph (max over ranks); engine state is restored."""
    us = float("inf")
    with preserved(eng._state()):
        try:
            g = eng._capture(nsteps)
        except Exception as e:  # same code on every rank: every rank lands here
            print(f"[csed] step-graph capture failed while timing ({e!r})", file=sys.stderr)
            _clear_hip_error()
            g = None
        if g is not None:
            g.replay()
            torch.cuda.synchronize(eng.device)
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(reps):
                g.replay()
            b.record()
            b.synchronize()
            us = a.elapsed_time(b) * 1e3 / (reps * nsteps)
            del g
    t = torch.tensor([us], dtype=torch.float64, device=_comm.ctl_device(eng.ctx))
    _comm.ctl_all_reduce(eng.ctx, t, dist.ReduceOp.MAX)
    return float(t.item())
