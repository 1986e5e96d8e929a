"""What replays a training step: the key of its launches, HIP-graph capture, and the HIP runtime calls
torch does not expose.  No engine logic: ``engine/fused.py`` describes a step as a list of launches
(``FusedLeNetTrainer._step_launches``) and hands its step callable and state here."""
from __future__ import annotations

import contextlib
import os
import time

import torch

from ..parallel import comm as _comm

_HIP_LIBS: list | None = None


def _hip_libs() -> list:
    """ctypes handles of the HIP runtime this process already loaded (via torch), never a second
    copy."""
    global _HIP_LIBS
    if _HIP_LIBS is None:
        import ctypes

        try:
            with open("/proc/self/maps") as f:
                paths = {ln.split()[-1] for ln in f if "libamdhip64.so" in ln}
            _HIP_LIBS = [ctypes.CDLL(p) for p in sorted(paths)]
        except OSError:
            _HIP_LIBS = []
    return _HIP_LIBS


def _clear_hip_error() -> None:
    """Reset this thread's sticky HIP error after a failed stream capture.  Our ops report
    ``hipGetLastError()`` after each launch, so an invalidated capture would otherwise
    surface as a failure of the next (eager) launch."""
    for lib in _hip_libs():
        lib.hipGetLastError()


class NativeGraph:
    """A step graph captured with ``torch.classes.csed.HipGraph`` (csrc/bindings.cpp), replayed by
    one ctypes ``hipGraphLaunch`` on the current stream (the ScriptObject keeps the graph alive)."""

    _launch = None

    def __init__(self, obj, device: torch.device):
        import ctypes

        self.obj = obj
        self.device_index = device.index
        self.exec = ctypes.c_void_p(obj.exec_handle())
        if NativeGraph._launch is None:
            fn = _hip_libs()[0].hipGraphLaunch
            fn.argtypes, fn.restype = [ctypes.c_void_p, ctypes.c_void_p], ctypes.c_int
            NativeGraph._launch = fn

    def replay(self) -> None:
        e = NativeGraph._launch(self.exec, torch._C._cuda_getCurrentRawStream(self.device_index))
        if e != 0:
            raise RuntimeError(f"hipGraphLaunch failed ({e})")

    def num_nodes(self) -> int:
        return int(self.obj.num_nodes())


def _hip_graph_upload(exec_handle: int, stream: int) -> bool:
    """hipGraphUpload of an instantiated graph on a stream (CSED_GRAPH_UPLOAD=1)."""
    import ctypes

    fn = _hip_libs()[0].hipGraphUpload
    fn.argtypes, fn.restype = [ctypes.c_void_p, ctypes.c_void_p], ctypes.c_int
    return fn(ctypes.c_void_p(exec_handle), ctypes.c_void_p(stream)) == 0


def launch_key(args):
    """What a captured graph or a native executor built from ``args`` points at and holds, hashable: a
    tensor is its (address, element count, dtype), a tuple or list (an argument list, a ``(name, args)``
    launch, a step's launches) the tuple of its items' keys, anything else (None, a number, a name)
    itself.  Equal keys replay the same launches.  Reads no device memory."""
    if isinstance(args, torch.Tensor):
        return (args.data_ptr(), args.numel(), args.dtype)
    if isinstance(args, (tuple, list)):
        return tuple(launch_key(a) for a in args)
    return args


def graph_plan(k: int, steps_per_graph: int) -> list[int]:
    """Graph sizes that run k steps: whole graphs of min(spg, k) steps, then one graph for
    the remainder (never a run of 1-step replays)."""
    if k <= 0:
        return []
    spg = max(1, min(steps_per_graph, k))
    full, rem = divmod(k, spg)
    return [spg] * full + ([rem] if rem else [])


@contextlib.contextmanager
def preserved(tensors):
    """Run the block, then put back the values ``tensors`` had on entry (also after an exception) and
    wait for the device."""
    saved = [t.clone() for t in tensors]
    try:
        yield
    finally:
        for t, v in zip(tensors, saved):
            t.copy_(v)
        for dev in {t.device for t in tensors if t.is_cuda}:
            torch.cuda.synchronize(dev)


def capture(step, nsteps: int, stream: torch.cuda.Stream, state, stamp):
    """Capture ``nsteps`` calls of ``step`` on ``stream`` into a HIP graph.

    ``state``: the device tensors a step advances, where this kind of step has not run on the capture
    stream yet, else None.  One eager warm-up step then runs there first (lazy RCCL communicator set-up,
    each kernel's first-launch symbol lookup -- neither may happen inside a capture), the state
    snapshotted before and restored after it.  The capture calls capture_begin / capture_end directly:
    ``torch.cuda.graph``'s device synchronize and ``empty_cache`` are not needed (the steps allocate
    nothing).

    ``CSED_NATIVE_GRAPH=1`` captures a native HIP graph instead (``torch.classes.csed.HipGraph``,
    replayed by a ctypes hipGraphLaunch): it skips torch's capture_begin generator set-up (a
    torch fill kernel, ~5 ms of first-launch code-object load in the reference span), but
    measured on one box its replays start later -- 14.9-15.7 vs 14.1-14.5 us per step in the
    driver's 20-step window, 13.34 vs 13.26 us at 3000 steps (profiles/r6/graph_ab.log) -- so
    torch's graphs stay the default.  ``CSED_GRAPH_UPLOAD=1`` uploads each graph after its
    instantiation (no measured effect on the first replay).  Host seconds go to ``stamp(key, dt)``:
    capture.warmup(.snapshot/.step/.sync/.restore) / .record / .instantiate / .upload."""
    device = stream.device
    cur = torch.cuda.current_stream(device)
    t0 = time.perf_counter()
    if state is not None:
        # snapshot the state the capture warm-up will advance; the side stream must
        # wait for the snapshot copies too (they are enqueued on the current stream)
        with preserved(state):
            stream.wait_stream(cur)
            tb = time.perf_counter()
            with torch.cuda.stream(stream):
                step()
            cur.wait_stream(stream)
            tc = time.perf_counter()
            torch.cuda.synchronize(device)
            td = time.perf_counter()
        te = time.perf_counter()
        for k, dt in (("snapshot", tb - t0), ("step", tc - tb), ("sync", td - tc), ("restore", te - td)):
            stamp(f"capture.warmup.{k}", dt)
    t1 = time.perf_counter()
    _comm.quiesce()  # (no pending collective for the watchdog to query during the capture)
    # thread_local: only this thread's unsafe calls invalidate the capture.  The process
    # group's watchdog thread keeps querying the events of earlier collectives while a step
    # that contains an RCCL all-reduce is captured; in the default (global) mode that query
    # invalidates the capture and the watchdog then aborts the process (seen on the GPU box,
    # profiles/round5.md)
    if os.environ.get("CSED_NATIVE_GRAPH") == "1":
        ng = torch.classes.csed.HipGraph()  # (csrc/bindings.cpp)
        with torch.cuda.stream(stream):
            ng.begin(device.index)
            try:
                for _ in range(nsteps):
                    step()
            finally:
                ng.end()  # (ends the capture even after a failed step; raises if it was invalidated)
        t2 = t3 = time.perf_counter()  # (end() instantiated it)
        if os.environ.get("CSED_GRAPH_UPLOAD", "0") == "1":
            with torch.cuda.stream(cur):
                ng.upload()
        g = NativeGraph(ng, device)
    else:
        g = torch.cuda.CUDAGraph(keep_graph=True)
        with torch.cuda.stream(stream):
            g.capture_begin(capture_error_mode="thread_local")
            try:
                for _ in range(nsteps):
                    step()
            finally:
                g.capture_end()
        t2 = time.perf_counter()
        g.instantiate()
        t3 = time.perf_counter()
        if os.environ.get("CSED_GRAPH_UPLOAD", "0") == "1":
            _hip_graph_upload(g.raw_cuda_graph_exec(), cur.cuda_stream)
    t4 = time.perf_counter()
    for k, dt in (("warmup", t1 - t0), ("record", t2 - t1), ("instantiate", t3 - t2), ("upload", t4 - t3)):
        stamp(f"capture.{k}", dt)
    return g
