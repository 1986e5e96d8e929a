"""Fused LeNet training engine: the MI355X fast path for ``Net`` (ref src/model.py).

One training step = two HIP kernels (``csed::lenet_train`` + ``csed::lenet_update``,
see csrc/kernels/lenet_fused.hip) at any world size:

    lenet_train    per-sample fwd+bwd of the whole network in LDS -> per-WG gradient slabs
    lenet_update   fixed-order slab reduce -> [world > 1: in-kernel exchange with every
                   peer over xGMI, rank-ordered sum] -> SGD-momentum + fp32 master params
                   + 16-bit weight images + device counters

The data-parallel gradient all-reduce (ref src/train_dist.py:83, DDP's one
87,360-byte bucket) is fused into lenet_update: each update lane pushes its
rank-local gradient value straight into every peer's IPC-mapped receive buffer
and sums what the peers pushed (csrc/comm buffers, LL-tagged words).  Its
bring-up and path timing are in engine/exchange_bringup.py; where it is off the
step runs as lenet_update (reduce only) -> RCCL all-reduce -> SGD kernel.

All per-step state (batch cursor into this rank's epoch permutation, Philox
offset, optimizer step) lives on the device, so a sequence of steps is
captured once into a HIP graph and replayed with no host work per step
(engine/replay.py).  A step is described once, as the list of its launches
(``_step_launches``): that list is what runs, and its ``launch_key`` is what the
cached graphs and the native executor are looked up by.

The model's parameters are re-homed into the engine's flat fp32 buffer, so the
``Net`` module always sees the current weights (checkpointing, evaluation
through the op library, ``state_dict()``) without copies.
"""
from __future__ import annotations

import functools
import math
import os
import sys
from collections import namedtuple
from typing import NamedTuple

import torch
import torch.distributed as dist

from ..data.mnist import MNIST_MEAN, MNIST_STD, MNISTData
from ..models.net import N_PARAMS, Net
from ..ops import _native
from ..parallel import comm as _comm
from ..parallel.comm import DistContext
from ..parallel import ipc as _ipc
from ..parallel.ipc import allreduce_mode, open_loopback_exchange, wait_timeout_s
from ..utils.flat import FlatParams
from . import exchange_bringup as _bringup
from . import replay as _replay
from .replay import launch_key


class LenetLayout(NamedTuple):
    """Buffer sizes and batch thresholds of the fused kernels: ``csed::lenet_layout()``'s values, in its order."""
    wimg_elems: int  # 16-bit weight-image elements (I_END)
    conv_params: int  # conv slab row per workgroup (CNP_PAD: conv1.w/b + conv2.w/b = 5280 floats in 64-float chunks)
    vec_len: int  # per-sample fc vector length (VEC)
    n_params: int  # flat parameters
    stage_max_batch: int  # largest per-rank batch that uses batch staging (STAGE_MAXB)
    exch_words: int  # 8-byte words per sender of lenet_update's fused exchange buffer
    split_k: int  # workgroups per sample of the split step (csed::lenet_train KS)
    tile_samples: int  # samples per tile of the sample-tile training kernel (csrc/kernels/lenet_tile.hip)
    tile_min_batch: int  # smallest per-rank batch the auto mode runs on the sample-tile kernel
    fc_part_elems: int  # floats of lenet_update's split-K fc scratch (partial sums, then the tiles' arrival counters)
    fc_tiles: int  # lenet_update's FC tiles (one arrival counter each)
    conv_blocks: int  # lenet_update's CONV blocks (they follow the launch's FC blocks)
    fc_counters_off: int  # float offset of the fc_tiles int32 arrival counters inside the scratch
    fc_part_min_batch: int  # per-rank batch from which the engine allocates the scratch


@functools.lru_cache(maxsize=None)
def lenet_layout() -> LenetLayout:
    _native.require()
    lay = LenetLayout(*(int(v) for v in torch.ops.csed.lenet_layout()))
    assert lay.n_params == N_PARAMS
    return lay


PER_SAMPLE, TILE, FP32 = 0, 1, 2  # LenetPlan.kernel
STRIDED, STAGED, SPLIT = 0, 1, 2  # LenetPlan.variant
KERNEL_NAMES = ("lenet_train", "lenet_tile", "lenet_train_f32")


class LenetPlan(NamedTuple):
    """What one ``csed::lenet_train`` / ``lenet_eval`` launch runs: ``csed::lenet_plan``'s values, in its order
    (csrc/kernels/lenet_plan.h, the rule the launchers themselves dispatch on)."""
    kernel: int  # PER_SAMPLE, TILE or FP32
    variant: int  # STRIDED over samples (tiles), one STAGED sample per workgroup, or the SPLIT step
    grid: int
    one_tile: int  # tile kernel: every workgroup has exactly one tile
    stage_rows: int  # staging rows the launch reads and writes (0: it gathers through perm)
    error: str  # "" for a valid launch, else the rule it breaks


UPDATE_SGD, UPDATE_EXCHANGE, UPDATE_SPLIT_K, UPDATE_PLAIN = 0, 1, 2, 3  # LenetUpdatePlan.form


class LenetUpdatePlan(NamedTuple):
    """What one ``csed::lenet_update`` launch runs: ``csed::lenet_update_plan``'s values, in its order
    (csrc/kernels/lenet_plan.h, the rule the launcher itself dispatches on)."""
    form: int  # UPDATE_SGD (lenet_sgd_kernel on grad_in), else lenet_update_kernel: UPDATE_EXCHANGE / SPLIT_K / PLAIN
    world_bound: int  # the exchange's world rounded up to 2 / 4 / 8 (0: no exchange)
    loopback: int
    sched: int  # the learning rate comes from the device-resident schedule
    blocks: int  # the grid: fc_blocks FC blocks, then the layout's conv_blocks
    fc_blocks: int
    waves_per_tile: int  # waves that split one FC tile's K
    tiles_per_block: int
    slices: int  # split-K batch slices per FC tile (1: unsplit)
    fc_tpb: int  # the kernel's trailing arguments: tiles per block fixed by the launcher (0: derived from B) ...
    fc_sl: int  # ... and the slices
    error: str  # "" for a valid launch, else the rule it breaks


class LenetGeometry(NamedTuple):
    """The engine's default full step at a per-rank batch: ``csed::lenet_geometry``'s values, in its order."""
    grid: int
    split: int  # the split step (split_k workgroups per sample)
    staged: int  # a staged batch of one row per workgroup
    tile_staged: int  # the tile kernel, staging every workgroup's first tile
    stage_rows: int


@functools.lru_cache(maxsize=None)
def lenet_plan(B: int, grid: int, mfma: int, kernel: int = 0, staged: bool = False, stage_next: bool = False,
               cursor: bool = True, train: bool = True) -> LenetPlan:
    """The plan of a launch (``kernel``: the request, 0 auto / 1 per sample / 2 tile).  No GPU needed."""
    _native.require()
    values, error = torch.ops.csed.lenet_plan(B, grid, mfma, kernel, staged, stage_next, cursor, train)
    return LenetPlan(*(int(v) for v in values), error)


def lenet_geometry(B: int, mfma: int, grid: int = 0, allow_split: bool = True) -> LenetGeometry:
    """The default geometry at per-rank batch B (``grid`` 0: min(B, 256)).  No GPU needed."""
    _native.require()
    return LenetGeometry(*(int(v) for v in torch.ops.csed.lenet_geometry(B, mfma, grid, allow_split)))


def lenet_update_plan(B: int, *, apply_sgd: bool = True, grad_in: bool = False, vslab: bool = True, exch_world: int = 0,
                      exch_loopback: bool = False, exch_cap: int | None = None, exch_timeout: bool = True,
                      lr_table: bool = False, lr_pos: bool | None = None, ticket: bool = True, lr_len: int | None = None,
                      fc_part_n: int = 0, forced_slices: int = -1) -> LenetUpdatePlan:
    """The plan of a ``csed::lenet_update`` launch at per-rank batch B, from what the launcher looks at: which
    optional arguments are set, the exchange's world (0: none), loopback flag and words per sender (default: the
    layout's), the schedule's length, the floats of the split-K scratch (0: none) and the forced slice count
    (default -1: this process's CSED_FC_SLICES, as the launcher reads it).  No GPU needed."""
    _native.require()
    values, error = torch.ops.csed.lenet_update_plan(
        B, apply_sgd, grad_in, vslab, exch_world, exch_loopback,
        lenet_layout().exch_words if exch_cap is None else exch_cap, exch_timeout, lr_table,
        lr_table if lr_pos is None else lr_pos, ticket, int(lr_table) if lr_len is None else lr_len, fc_part_n,
        forced_slices)
    return LenetUpdatePlan(*(int(v) for v in values), error)


@functools.lru_cache(maxsize=None)
def tile_grid(B: int) -> int:
    """Workgroups of the sample-tile kernel at per-rank batch B."""
    _native.require()
    return int(torch.ops.csed.lenet_tile_grid(B))


# Argument names of a step's two launches in the order of their op schemas (csrc/bindings.cpp; LenetStepper's
# set_train / set_update take the same lists): filled in by FusedLeNetTrainer.train_args / update_args alone.
TRAIN_FIELDS = ("images", "labels", "perm", "cursor", "B", "rank", "wimg", "params", "slab", "vslab", "loss_parts",
                "grad_scale", "mean", "std", "drop_p", "seed", "rng_offset", "grid", "mfma_dtype", "dbg", "xstage",
                "lstage", "stage_next", "kernel")
UPDATE_FIELDS = ("slab", "grid", "vslab", "B", "grad_in", "grad_out", "params", "momentum", "wimg", "lr", "mom",
                 "dampening", "weight_decay", "nesterov", "step", "ticket", "cursor", "rng_offset", "apply_sgd",
                 "loss_parts", "nparts", "loss_acc", "mfma_dtype", "dbg", "exch_id", "exch_timeout_s", "grad_post",
                 "fc_part", "lr_table", "lr_pos", "ema", "ema_decay")
# What ``csed::lenet_update_adam`` (LenetStepper.set_update_adam) takes behind UPDATE_FIELDS: Adam's exp_avg_sq
# and constants (exp_avg lives in ``momentum``); ``decoupled``: AdamW.
ADAM_FIELDS = ("adam_v", "beta1", "beta2", "eps", "decoupled")
TrainArgs = namedtuple("TrainArgs", TRAIN_FIELDS)
UpdateArgs = namedtuple("UpdateArgs", UPDATE_FIELDS, defaults=(None, 0.0))  # (the moving average: off)
AdamArgs = namedtuple("AdamArgs", ADAM_FIELDS)
UpdateAdamArgs = namedtuple("UpdateAdamArgs", UPDATE_FIELDS + ADAM_FIELDS)  # (one lenet_update_adam launch)
OPTIMIZERS = ("sgd", "adam", "adamw")
_ENGINE = object()  # (default of a builder's ``cursor``: the engine's own device cursor)


def native_max_steps() -> int:
    """Longest run of full steps launched by the native executor instead of a graph replay
    (``CSED_NATIVE_STEPS``; 0 = always graphs).  See ``FusedLeNetTrainer.step_plan``."""
    return int(os.environ.get("CSED_NATIVE_STEPS", "0"))


class FusedLeNetTrainer:
    def __init__(self, model: Net, train: MNISTData, lr: float = 0.01, momentum: float = 0.5,
                 dampening: float = 0.0, weight_decay: float = 0.0, nesterov: bool = False,
                 global_batch: int = 64, ctx: DistContext | None = None,
                 compute_dtype: torch.dtype = torch.bfloat16, drop_p: float = 0.5, seed: int = 1,
                 grid: int | None = None, broadcast_init: bool = True, comm: bool | None = None,
                 split: bool | None = None, loopback_world: int = 0,
                 reuse_exchange: "FusedLeNetTrainer | None" = None, optimizer: str = "sgd",
                 betas: tuple[float, float] = (0.9, 0.999), eps: float = 1e-8):
        import time

        _native.require()
        t_init = time.perf_counter()
        self.bringup_s: dict[str, float] = {}  # bring-up phases (s), for the bench JSON
        self.ctx = ctx or DistContext(device=next(model.parameters()).device)
        self.device = self.ctx.device
        if self.device.type != "cuda":
            raise RuntimeError("FusedLeNetTrainer runs on a GPU")
        self.model = model
        self.world = self.ctx.world_size if self.ctx.is_distributed else 1
        # comm=True forces the all-reduce path even at world size 1 (tests RCCL graph capture
        # on a single GPU); default: collectives exactly when there is more than one rank
        self.comm = (self.world > 1) if comm is None else (bool(comm) and dist.is_initialized())
        if global_batch % self.world:
            raise ValueError(f"global batch {global_batch} not divisible by world size {self.world}")
        self.global_batch = int(global_batch)
        self.B = self.global_batch // self.world
        if compute_dtype not in _native.MFMA_CODE:
            raise ValueError(f"compute dtype {compute_dtype}: expected bfloat16, float16 or float32")
        lay = lenet_layout()
        self.fp32 = compute_dtype == torch.float32
        self.mfma = _native.MFMA_CODE[compute_dtype]
        # The step's geometry (csrc/kernels/lenet_plan.h lenet_geometry).  Batch staging (one workgroup
        # per sample): lenet_update gathers the next step's pixels + labels one step ahead, so lenet_train
        # starts with no dependent index chain.  Split step (lenet_fused.hip / lenet_fused_f32.hip KS > 1):
        # split_k workgroups per sample share the backward conv stages; used whenever the whole grid fits
        # one wave of the GPU.  CSED_SPLIT=0 keeps one workgroup per sample.  The exact-fp32 kernel gathers
        # its samples itself and stages its batch only in the split step.  The sample-tile kernel (16-bit
        # large batches, csrc/kernels/lenet_tile.hip) stages the first tile of every workgroup instead.
        auto = os.environ.get("CSED_SPLIT", "auto").strip().lower() != "0"
        geo = lenet_geometry(self.B, self.mfma, int(grid) if grid else 0,
                             grid is None and (auto if split is None else bool(split)))
        self.grid, self.split, self.staged = geo.grid, bool(geo.split), bool(geo.staged)
        self.tile_staged = bool(geo.tile_staged)
        self.lr, self.momentum, self.dampening = float(lr), float(momentum), float(dampening)
        self.weight_decay, self.nesterov = float(weight_decay), bool(nesterov)
        # "adam" / "adamw": the launches that apply the gradient run torch.optim.Adam's / AdamW's rule on the
        # device (csed::lenet_update_adam) instead of SGD's; ``momentum``, ``dampening`` and ``nesterov`` are
        # SGD's and are not passed then
        if optimizer not in OPTIMIZERS:
            raise ValueError(f"optimizer {optimizer!r}: expected one of {OPTIMIZERS}")
        self.optimizer = optimizer
        self.betas, self.eps = (float(betas[0]), float(betas[1])), float(eps)
        if self.adam and (not all(0.0 <= b < 1.0 for b in self.betas) or not self.eps > 0.0):
            raise ValueError(f"betas {betas} / eps {eps}: expected 0 <= beta < 1 and eps > 0")
        self.compute_dtype = compute_dtype
        self.drop_p = float(drop_p)
        self.seed = int(seed)  # masks decorrelate across ranks through the rank id in the element index
        self.train_data = train.to(self.device)
        dev = self.device
        self.bringup_s["data_to_device"] = time.perf_counter() - t_init

        self.flat = FlatParams(list(model.parameters()))
        if self.flat.numel != N_PARAMS:
            raise ValueError("FusedLeNetTrainer needs the reference Net architecture")
        if broadcast_init and self.world > 1:  # the DDP-constructor parameter sync (CS4)
            _comm.ctl_broadcast(self.ctx, self.flat.data, src=0)  # (RCCL, or the host over gloo)
        self.momentum_buf = _native.zeros(self.flat.data.shape, torch.float32, self.flat.data.device)
        # Adam's exp_avg_sq (exp_avg lives in momentum_buf); the extension's own fill, like every buffer here
        self.adam_v = (_native.zeros(self.flat.data.shape, torch.float32, self.flat.data.device)
                       if self.adam else None)
        # zero-initialised: padding rows / columns of the images must stay zero
        self.wimg = _native.zeros(lay.wimg_elems, torch.int16, dev)
        # per-WG conv partial gradients and per-sample fc vectors (see lenet_fused.hip)
        self.slab = torch.empty((self.grid, lay.conv_params), dtype=torch.float32, device=dev)
        # (fp32 [B, 464] for the exact-fp32 kernel; the 16-bit kernels keep raw 16-bit values
        # feature-major, [464, round_up(B, 64)], in the same bytes: fc_vectors() decodes either)
        self.vslab = _native.zeros(((self.B + 63) // 64 * 64, lay.vec_len), torch.float32, dev)
        self.loss_parts = _native.zeros(2 * self.grid, torch.float32, dev)
        self.loss_acc = _native.zeros(2, torch.float32, dev)  # running (loss sum, correct)
        self.step_count = _native.zeros(1, torch.long, dev)
        self.ticket = _native.zeros(1, torch.int32, dev)
        self.cursor = _native.zeros(1, torch.long, dev)
        self.rng_offset = _native.zeros(1, torch.long, dev)
        self.eval_parts = _native.zeros(2 * 256, torch.float32, dev)
        self.perm = _native.arange(self.B, dev)
        # split-K fc-gradient scratch (lenet_plan.h lenet_update_plan): per-rank batches from
        # fc_part_min_batch without the fused exchange form the fc weight gradients as up to 8 batch
        # slices per tile on all CUs, the tile's last slice finishing it (8 x 88 tiles x 256 partial
        # sums, then 88 arrival counters that must start at zero)
        self.fc_part = (_native.zeros((lay.fc_part_elems + 127) // 128 * 128, torch.float32, dev)
                        if self.B >= lay.fc_part_min_batch else None)
        # one staging row per workgroup (split step: row r holds sample r % B), or the tile kernel's
        # grid * tile_samples rows
        srows = geo.stage_rows
        self.xstage = _native.zeros((srows, 784), torch.uint8, dev) if srows else None
        self.lstage = _native.zeros(srows, torch.long, dev) if srows else None
        t_mark = time.perf_counter()
        self.repack()  # (the extension's first kernel launch: its code object loads here)
        self.bringup_s["first_kernel"] = time.perf_counter() - t_mark
        # both caches are keyed on launch_key of the launches they replay; invalidate() empties them
        self._graphs: dict[tuple, object] = {}  # torch.cuda.CUDAGraph (or replay.NativeGraph), see graph()
        self._warmed: set[str] = set()  # step kinds whose capture warm-up has run (see _capture)
        self._cap_stream: torch.cuda.Stream | None = None
        self._stepper: tuple | None = None  # (key, csed.LenetStepper), see stepper()
        self.lr_schedule = None  # optim.LRSchedule on the device (set_lr_schedule), or None: constant self.lr
        self.ema: torch.Tensor | None = None  # the parameters' moving average (set_ema), or None: off
        self.ema_decay = 0.0
        self._ema_wimg: torch.Tensor | None = None  # its weight image, packed for evaluate(ema=True)
        self.native_max = native_max_steps()
        # which training kernel a step asks for: 0 auto (the sample-tile kernel, csrc/kernels/lenet_tile.hip,
        # for large 16-bit per-rank batches), 1 the per-sample lenet_train, 2 the sample-tile kernel
        self.train_kernel = 0
        self._eval_cache: dict[int, tuple] = {}
        self._order_host: torch.Tensor | None = None
        self.capture_comm_ok: bool | None = None
        # gradient all-reduce.  Preferred: the exchange fused into lenet_update (see the module
        # docstring).  Fallback step (3 kernels: reduce-only update -> RCCL all-reduce -> SGD).
        self.exch = None
        self.exchange_note: str | None = None  # why the data-parallel step runs as it does (reports)
        self.exch_timeout_s = wait_timeout_s()
        self.path_timing_us: dict | None = None
        self._xdiag: dict = {}  # stage results of the exchange bring-up (exchange_diag)
        self._path_pending: str | None = None  # a deferred path timing (select_path)
        self.loopback_world = 0  # (set below; the exchange bring-up's reports read it)
        multi = self.comm and self.world > 1
        mode = allreduce_mode() if multi else "rccl"
        donor = reuse_exchange if (multi and reuse_exchange is not None and reuse_exchange.exch is not None
                                   and not reuse_exchange.loopback_world) else None
        if donor is not None:
            # another engine's exchange, already opened, self-tested and timed on this process
            # group (bench.py's fp32 sub-record after the 16-bit run): the IPC buffer carries
            # fp32 gradient words whatever the compute dtype, and its per-workgroup tags continue
            # on every rank alike.  The donor gives it up (its close() no longer frees it).
            self.exch, donor.exch = donor.exch, None
            self._xdiag = dict(donor._xdiag)
            self.path_timing_us = donor.path_timing_us
            self.exchange_note = "fused exchange reused from the previous engine (opened and self-tested there)"
        elif multi:
            self._xdiag["ranks_per_gpu"] = _ipc.ranks_per_gpu(self.ctx)  # (collective: every rank)
            if mode in ("auto", "fused"):
                _bringup.enable_exchange(self, required=(mode == "fused"))
            else:
                self._xdiag["ipc_open"] = f"not tried (CSED_ALLREDUCE={mode})"
        # Loopback exchange (one GPU, no process group): lenet_update runs its full push + poll
        # code for loopback_world - 1 virtual peers that are slots of this rank's own buffer
        # (csrc/comm ipc_open_loopback).  Each peer returns this rank's own gradient, and the
        # loss is scaled by 1 / (loopback_world * global batch), so the summed gradient is this
        # rank's batch mean: the same training math as world 1, at the per-step kernel cost of a
        # world-N exchange minus the xGMI flight time (the per-rank step of the driver's N-GPU
        # run, measured on one GPU: bench.py --loopback-world N).
        self.loopback_world = int(loopback_world) if loopback_world and int(loopback_world) > 1 else 0
        if self.loopback_world:
            if self.world > 1:
                raise ValueError("loopback_world is a one-GPU measurement mode (world size 1)")
            self.exch = open_loopback_exchange(self.device, lay.exch_words, self.loopback_world)
            self.exchange_note = f"loopback exchange: {self.loopback_world} virtual ranks on one GPU"

    @property
    def adam(self) -> bool:
        """Whether the engine trains with Adam / AdamW (``optimizer``) instead of SGD."""
        return self.optimizer != "sgd"

    @property
    def grad_scale(self) -> float:
        """Loss-gradient scale of a full step: 1 / (global batch) (x 1 / loopback_world)."""
        return 1.0 / (self.global_batch * max(1, self.loopback_world))

    def _vec16(self, B: int) -> torch.Tensor:
        """The 16-bit kernels' fc-vector slab of a batch of B: raw [round_up(B, 64) / 4, 464, 4]
        (sample quads, kernels/lenet_layout.h)."""
        q, nv = (B + 63) // 64 * 16, lenet_layout().vec_len
        return self.vslab.view(-1).view(torch.int16)[:q * nv * 4].view(q, nv, 4)

    def fc_vectors(self, B: int | None = None) -> torch.Tensor:
        """The step's per-sample fc vectors (P2 | dZ1 | H | dlogits) as fp32 [B, 464], decoded
        from either slab layout (kernels/lenet_layout.h)."""
        B = self.B if B is None else int(B)
        if self.fp32:
            return self.vslab[:B].clone()
        v = self._vec16(B).transpose(1, 2).reshape(-1, lenet_layout().vec_len)[:B]  # [quad, 4, 464] -> [sample, 464]
        return v.contiguous().view(self.compute_dtype).float()

    def set_fc_vectors(self, v: torch.Tensor) -> None:
        """Fill the fc-vector slab from fp32 [B, 464] values (rounded to the compute dtype)."""
        B = v.shape[0]
        self.vslab.zero_()
        if self.fp32:
            self.vslab[:B].copy_(v)
            return
        nv = lenet_layout().vec_len
        buf = torch.zeros(((B + 63) // 64 * 64, nv), dtype=self.compute_dtype, device=self.device)
        buf[:B] = v.to(device=self.device, dtype=self.compute_dtype)
        self._vec16(B).copy_(buf.view(torch.int16).view(-1, 4, nv).transpose(1, 2))

    @property
    def allreduce_kind(self) -> str:
        if self.loopback_world:
            return f"fused-ipc-loopback{self.loopback_world}"
        if not self.comm:
            return "none"
        if self.exch is not None:
            return "fused-ipc"
        return "rccl"

    # ------------------------------------------------- fused gradient exchange
    def select_path(self) -> bool:
        """Run the fused-vs-RCCL step timing deferred by a lazy-RCCL bring-up (collective; a no-op
        otherwise).  True if the step path changed (the cached graphs are dropped then)."""
        tp, self._path_pending = self._path_pending, None
        if tp is None or self.exch is None:
            return False
        _bringup.select_path_now(self, tp)
        if self.exch is None:
            self.invalidate()
            return True
        return False

    def exchange_diag(self) -> dict:
        """This rank's data-parallel diagnostics (``parallel/ipc.py`` DIAG_KEYS)."""
        return _bringup.exchange_diag(self)

    def invalidate(self) -> None:
        """Drop (and free) the captured graphs and the native executor.  Their keys follow every change
        the step's arguments show; this is for the ones they cannot show -- an exchange remapped behind
        the same id, an epoch order of another length taking ``perm``'s place -- and for letting go of
        what will not be replayed again."""
        self._graphs.clear()
        self._stepper = None

    def close(self) -> None:
        """Release the graphs and the IPC buffers (collective on every rank: a barrier runs
        first so that no peer is still pushing into this rank's buffers)."""
        self.invalidate()
        if self.loopback_world and self.exch is not None:  # local buffer, no peers
            torch.cuda.synchronize(self.device)
            self.exch.close()
            self.exch = None
        if self.exch is not None and dist.is_initialized():
            torch.cuda.synchronize(self.device)
            _comm.barrier(self.ctx)
        if self.exch is not None:
            self.exch.close()
        self.exch = None

    def comm_errors(self) -> int:
        """Nonzero if the IPC exchange ever timed out waiting for a peer (bit 0) or, looped back,
        received a word whose value was not the one pushed (bit 1; see ``comm_diag``).
        Synchronous."""
        return self.exch.error() if self.exch is not None else 0

    def comm_diag(self) -> dict | None:
        """The first in-kernel loopback mismatch record (block, peer row, word, tag, got, want)."""
        return self.exch.diag() if self.exch is not None else None

    def inject_exchange_fault(self, on: bool = True) -> None:
        """Fault injection (tests, ``--inject-exchange-fault``): this rank's exchange pushes go
        to a private dead-end buffer (csrc/comm ipc_set_mute), so to its peers -- or, in
        loopback mode, to itself -- it is a dead rank whose words never arrive: their waits run
        into CSED_IPC_TIMEOUT_S and raise the error word.  Captured graphs and the native
        executor hold the old mapping, so both are dropped."""
        if self.exch is None:
            raise RuntimeError("no IPC exchange to inject a fault into")
        self.exch.mute(on)
        self.invalidate()

    # ----------------------------------------------------------------- state
    def repack(self) -> None:
        """Rebuild the 16-bit weight images from the fp32 master parameters."""
        torch.ops.csed.lenet_pack(self.flat.data, self.wimg, self.mfma)

    def set_epoch_order(self, order: torch.Tensor) -> None:
        """This rank's sample order for the epoch (int64 indices into the train set).

        A host order is uploaded asynchronously from pinned memory (the host never waits for
        the device here), so the next epoch's permutation can be prepared while the current
        epoch's graphs still run."""
        if order.numel() < self.B:
            raise ValueError("epoch order shorter than one batch")
        if order.device.type == "cpu":
            host = order.to(torch.long).contiguous().pin_memory()
            self._order_host = host  # alive until the copy below has run
            if host.numel() == self.perm.numel():  # straight into the captured buffer: one copy
                self.perm.copy_(host, non_blocking=True)
                _native.zero_(self.cursor)
                self._stage_current()
                return
            order = torch.empty(host.shape, dtype=torch.long, device=self.device)
            order.copy_(host, non_blocking=True)
        else:
            order = order.to(self.device, torch.long).contiguous()
        if order.numel() == self.perm.numel():
            self.perm.copy_(order)
        else:
            self.invalidate()  # captured pointers refer to the old buffer
            self.perm = order
        _native.zero_(self.cursor)
        self._stage_current()

    def _stage_current(self) -> None:
        """Gather the batch at the cursor into the staging buffers (epoch start)."""
        if self.xstage is not None:
            torch.ops.csed.lenet_stage(self.train_data.images, self.train_data.labels, self.perm, self.cursor,
                                       self.B, self.xstage, self.lstage)

    def uses_tile_kernel(self, B: int | None = None, grid: int | None = None) -> bool:
        """Whether a full step of per-rank batch B on ``grid`` workgroups runs the sample-tile kernel
        (csrc/kernels/lenet_tile.hip): the plan of kernel_for()'s request."""
        return self._plan(B, grid).kernel == TILE

    def _plan(self, B: int | None = None, grid: int | None = None, staged: bool = False) -> LenetPlan:
        """The plan of this engine's training launch of per-rank batch B on ``grid`` workgroups."""
        B, grid = self.B if B is None else B, self.grid if grid is None else grid
        return lenet_plan(B, grid, self.mfma, self.kernel_for(B, grid), staged)

    @property
    def kernel_names(self) -> str:
        """The HIP kernels of one full training step, as launched (reports)."""
        return KERNEL_NAMES[self._plan().kernel] + " + lenet_update"

    @property
    def step_kind(self) -> str:
        """How a full (staged) training step is launched."""
        return "two kernels" if (not self.comm or self.exch is not None) else "update split around an all-reduce"

    def steps_per_epoch(self) -> int:
        return math.ceil(self.perm.numel() / self.B)

    def full_steps(self) -> int:
        return self.perm.numel() // self.B

    # ------------------------------------------------------------ launches
    def train_args(self, *, B=None, grid=None, perm=None, cursor=_ENGINE, grad_scale=None, rank=None, dbg=None,
                   stage_next=False, staged=None, scale_in_kernel=None) -> TrainArgs:
        """The arguments of ``csed::lenet_train`` (TRAIN_FIELDS), by default the engine's full step: B samples
        at ``cursor`` in ``perm`` (``cursor=None``: perm's first B) on ``grid`` workgroups of kernel_for()'s
        kernel.  ``staged``: read the batch from the staging buffers (default: where that kernel stages a
        batch of the engine's own grid at a cursor); ``stage_next``: a staged launch gathers the next batch.
        ``grad_scale``: the step's loss-gradient scale.  16-bit steps run their backward at per-sample scale
        (dlogits = softmax - onehot, so fp16 gradient images stay normal numbers at any batch) and
        lenet_update applies it in fp32 (grad_post); the exact-fp32 kernel takes it in-kernel
        (``scale_in_kernel``).  For a power-of-two batch both give bit-identical bf16 results."""
        B, grid = self.B if B is None else B, self.grid if grid is None else grid
        cursor = self.cursor if cursor is _ENGINE else cursor
        kernel = self.kernel_for(B, grid)
        if staged is None:  # (the epoch's short tail, or a launch on another grid, reads perm)
            staged = self._stages(kernel) and cursor is not None and grid == self.grid
        grad_scale = self.grad_scale if grad_scale is None else grad_scale
        in_kernel = self.fp32 if scale_in_kernel is None else scale_in_kernel
        return TrainArgs(
            images=self.train_data.images, labels=self.train_data.labels, perm=self.perm if perm is None else perm,
            cursor=cursor, B=B, rank=self.ctx.rank if rank is None else rank, wimg=self.wimg, params=self.flat.data,
            slab=self.slab, vslab=self.vslab, loss_parts=self.loss_parts, grad_scale=grad_scale if in_kernel else 1.0,
            mean=MNIST_MEAN, std=MNIST_STD, drop_p=self.drop_p, seed=self.seed, rng_offset=self.rng_offset, grid=grid,
            mfma_dtype=self.mfma, dbg=dbg, xstage=self.xstage if staged else None,
            lstage=self.lstage if staged else None, stage_next=bool(stage_next and staged), kernel=kernel)

    def update_args(self, mode: str, *, B=None, grid=None, cursor=_ENGINE, grad=None, grad_scale=None, exchange=None,
                    dbg=None, with_loss=True, fc_split=None, scale_in_kernel=None) -> UpdateArgs:
        """The arguments of ``csed::lenet_update`` (UPDATE_FIELDS).  ``mode``: "step" (reduce the slabs, then
        SGD, in one kernel), "reduce" (reduce only, into ``grad``; advances neither cursor nor Philox offset)
        or "apply" (SGD from the already reduced ``grad``).  The launch that applies SGD ("step" / "apply") gets
        the learning-rate schedule's table and position where one is set (set_lr_schedule): it trains at
        its own step's entry and advances the position.  It also gets the moving average's buffer and decay
        (set_ema): the lane that writes a parameter updates its average.  The kernel that reduces also sums the loss
        partials (``with_loss``), applies the 16-bit steps' ``grad_scale`` (train_args), runs the fused
        exchange (``exchange``; default: where the engine has one) and, by default exactly without it, gets
        the split-K fc scratch of per-rank batches > 1024 (``fc_split``)."""
        if mode not in ("step", "reduce", "apply") or (grad is None) != (mode == "step"):
            raise ValueError(f"lenet_update mode {mode!r}: 'step', or 'reduce' / 'apply' with grad=")
        B, grid = self.B if B is None else B, self.grid if grid is None else grid
        reduces, advances = mode != "apply", mode != "reduce"
        exch = self.exch if reduces and (self.exch is not None if exchange is None else exchange) else None
        loss = reduces and with_loss
        grad_scale = self.grad_scale if grad_scale is None else grad_scale
        in_kernel = self.fp32 if scale_in_kernel is None else scale_in_kernel
        fc_split = (reduces and exch is None) if fc_split is None else fc_split
        sch = self.lr_schedule if advances else None
        sgd = not self.adam  # (SGD's own arguments are zero under Adam: the launcher insists)
        return UpdateArgs(
            slab=self.slab, grid=grid, vslab=self.vslab, B=B, grad_in=grad if mode == "apply" else None,
            grad_out=grad if mode == "reduce" else None, params=self.flat.data, momentum=self.momentum_buf,
            wimg=self.wimg, lr=self.lr, mom=self.momentum if sgd else 0.0, dampening=self.dampening if sgd else 0.0,
            weight_decay=self.weight_decay, nesterov=self.nesterov and sgd, step=self.step_count, ticket=self.ticket,
            cursor=(self.cursor if cursor is _ENGINE else cursor) if advances else None,
            rng_offset=self.rng_offset if advances else None, apply_sgd=advances,
            loss_parts=self.loss_parts if loss else None, nparts=grid if loss else 0,
            loss_acc=self.loss_acc if loss else None, mfma_dtype=self.mfma, dbg=dbg,
            exch_id=-1 if exch is None else exch.id, exch_timeout_s=2.0 if exch is None else self.exch_timeout_s,
            grad_post=grad_scale if reduces and not in_kernel else 1.0, fc_part=self.fc_part if fc_split else None,
            lr_table=None if sch is None else sch.table, lr_pos=None if sch is None else sch.pos,
            ema=self.ema if advances else None, ema_decay=self.ema_decay if advances and self.ema is not None else 0.0)

    def adam_args(self) -> AdamArgs:
        """What a launch that applies Adam / AdamW takes behind update_args (ADAM_FIELDS)."""
        return AdamArgs(adam_v=self.adam_v, beta1=self.betas[0], beta2=self.betas[1], eps=self.eps,
                        decoupled=self.optimizer == "adamw")

    def update_launch(self, mode: str, **kw) -> tuple:
        """The (name, arguments) launch of update_args(mode, ...): ``lenet_update``, or under Adam / AdamW, for
        the modes that apply the gradient ("step" / "apply"), ``lenet_update_adam`` with adam_args behind."""
        args = self.update_args(mode, **kw)
        if self.adam and mode != "reduce":
            return ("lenet_update_adam", UpdateAdamArgs(*args, *self.adam_args()))
        return ("lenet_update", args)

    def update_plan(self, args: UpdateArgs) -> LenetUpdatePlan:
        """The plan of the ``csed::lenet_update`` launch that ``args`` (update_args) describes."""
        exch = args.exch_id >= 0
        return lenet_update_plan(
            args.B, apply_sgd=args.apply_sgd, grad_in=args.grad_in is not None, vslab=args.vslab is not None,
            exch_world=(self.loopback_world or self.world) if exch else 0,
            exch_loopback=exch and bool(self.loopback_world), exch_timeout=args.exch_timeout_s > 0,
            lr_table=args.lr_table is not None, lr_pos=args.lr_pos is not None, ticket=args.ticket is not None,
            lr_len=0 if args.lr_table is None else args.lr_table.numel(),
            fc_part_n=0 if args.fc_part is None else args.fc_part.numel())

    def fc_counters(self) -> torch.Tensor:
        """The split-K scratch's per-tile arrival counters (an int32 view of fc_part; zero between launches)."""
        lay = lenet_layout()
        return self.fc_part[lay.fc_counters_off:lay.fc_counters_off + lay.fc_tiles].view(torch.int32)

    def _step_launches(self, perm: torch.Tensor | None = None, **kw) -> list[tuple]:
        """A step's launches on ``perm`` (default: the epoch order), in order, as (name, arguments): ops of
        the extension, and "all_reduce" on the flat gradient.  ``kw``: B, grid, cursor, grad_scale where not
        the full step's.  What _launch_step runs and what graph() keys on (replay.launch_key)."""
        # full steps read the staged batch and stage the next one; the epoch's short tail uses perm
        train = ("lenet_train", self.train_args(perm=perm, stage_next=True, **kw))
        if self.exch is not None or not self.comm:  # one kernel: the fused exchange, or no exchange at all
            return [train, self.update_launch("step", **kw)]
        g = self.flat.grad
        return [train, self.update_launch("reduce", grad=g, **kw), ("all_reduce", (g,)),
                self.update_launch("apply", grad=g, **kw)]

    def _tail_launches(self) -> list[tuple]:
        """The launches of the epoch's short last batch."""
        rem = self.tail_size()
        tail = self.perm[self.full_steps() * self.B:]  # a view: stable pointer for graph replay
        gb = rem * self.world * max(1, self.loopback_world)  # (the sampler pads to a multiple: same on every rank)
        # the tail step does not use the cursor; keep it consistent for the next epoch
        return (self._step_launches(tail, B=rem, grid=min(rem, self.grid), cursor=None, grad_scale=1.0 / gb)
                + [("lenet_add_", (self.cursor, 1))])

    @staticmethod
    def _launch_step(launches: list[tuple]) -> None:
        for name, args in launches:
            if name == "all_reduce":
                dist.all_reduce(*args, op=dist.ReduceOp.SUM)
            else:
                getattr(torch.ops.csed, name)(*args)

    def _stages(self, kernel: int) -> bool:
        """Whether a full step launched with ``kernel`` (kernel_for) reads / writes the staging
        buffers: the per-sample kernel's (one row per workgroup) or the tile kernel's (first tiles) --
        where the engine stages at all, a launch whose plan takes exactly the rows it keeps."""
        if not (self.staged or self.tile_staged):
            return False
        p = lenet_plan(self.B, self.grid, self.mfma, kernel, True)
        return not p.error and p.stage_rows == self.xstage.shape[0]

    def kernel_for(self, B: int, grid: int) -> int:
        """``train_kernel`` for a launch of per-rank batch B on ``grid`` workgroups: the tile kernel
        only where its grid (tile_grid) is the launch's, else per-sample."""
        if self.train_kernel == 0:
            return 0 if (B < lenet_layout().tile_min_batch or grid == tile_grid(B)) else 1
        if self.train_kernel == 2 and grid != tile_grid(B):
            return 1
        return self.train_kernel

    def gradient(self, grid: int | None = None, dbg: torch.Tensor | None = None) -> torch.Tensor:
        """Mean-loss gradient of the batch at the cursor, without updating anything
        (lenet_train + the reduce-only lenet_update).  Also accumulates the batch's
        loss / correct count into the running totals."""
        kw = dict(grid=grid or self.grid, grad_scale=1.0 / self.global_batch)  # (no loopback factor: no exchange)
        g = torch.empty(N_PARAMS, dtype=torch.float32, device=self.device)
        torch.ops.csed.lenet_train(*self.train_args(dbg=dbg, **kw))
        torch.ops.csed.lenet_update(*self.update_args("reduce", grad=g, exchange=False, **kw))
        return g

    def step(self) -> None:
        """One full-batch training step at the device cursor (eager launches)."""
        self._launch_step(self._step_launches())

    def tail_size(self) -> int:
        """Per-rank samples of the epoch's short last batch (0 if the epoch divides evenly)."""
        return self.perm.numel() - self.full_steps() * self.B

    def _tail_step(self) -> None:
        self._launch_step(self._tail_launches())

    def last_partial_step(self, use_graph: bool = True) -> None:
        """The epoch's final short batch (ref DataLoader drop_last=False semantics); replayed
        from its own captured graph like the full steps."""
        if self.tail_size() <= 0:
            return
        g = self.graph(1, tail=True) if use_graph and self.capture_comm_ok is not False else None
        if g is not None:
            g.replay()
        else:
            self._tail_step()

    # --------------------------------------------------------- graph capture
    def _state(self) -> list[torch.Tensor]:
        """Device tensors a training step advances."""
        return ([self.flat.data, self.momentum_buf, self.wimg, self.step_count, self.cursor, self.rng_offset,
                 self.loss_acc] + ([self.xstage, self.lstage] if self.xstage is not None else [])
                + ([self.lr_schedule.pos] if self.lr_schedule is not None else [])
                + ([self.ema] if self.ema is not None else [])
                + ([self.adam_v] if self.adam_v is not None else []))

    def _stamp(self, key: str, dt: float) -> None:
        self.bringup_s[key] = self.bringup_s.get(key, 0.0) + dt

    def _capture(self, nsteps: int, tail: bool = False):
        """Capture ``nsteps`` full steps (or the epoch's tail step) into a HIP graph (replay.capture) on
        the engine's capture stream.  The first capture of each step kind (full / tail x all-reduce path x
        kernel) warms the step up there."""
        import time

        t0 = time.perf_counter()
        if self._cap_stream is None:  # (one capture stream per engine: creating a stream costs ms)
            self._cap_stream = torch.cuda.Stream(self.device)
        kind = f"{'tail' if tail else 'full'}/{self.allreduce_kind}/{self.train_kernel}"
        self._stamp("capture.stream", time.perf_counter() - t0)
        g = _replay.capture(self._tail_step if tail else self.step, nsteps, self._cap_stream,
                            None if kind in self._warmed else self._state(), self._stamp)
        self._warmed.add(kind)
        return g

    def graph(self, nsteps: int, tail: bool = False):
        """The captured graph of ``nsteps`` full steps (or of the epoch's tail step), cached under what its
        launches point at and hold."""
        key = (nsteps, tail, launch_key(self._tail_launches() if tail else self._step_launches()))
        if key in self._graphs:
            return self._graphs[key]
        if self.allreduce_kind == "rccl" and dist.is_initialized() and dist.get_backend() == "gloo":
            # the process group's all-reduce runs on the host (gloo): nothing to capture
            self.capture_comm_ok = False
            return None
        try:
            g = self._capture(nsteps, tail)
            self.capture_comm_ok = True
        except Exception as e:  # RCCL capture unsupported -> eager fallback
            print(f"[csed] HIP graph capture failed ({e!r}); running steps eagerly", file=sys.stderr)
            self.capture_comm_ok = False
            _replay._clear_hip_error()
            torch.cuda.synchronize(self.device)
            return None
        self._graphs[key] = g
        return g

    graph_plan = staticmethod(_replay.graph_plan)

    def prepare(self, steps_per_graph: int = 16, ks: tuple[int, ...] = (), tail: bool = True) -> None:
        """Capture up front (capture is never inside a timed region) every graph that
        ``run_steps(k, steps_per_graph)`` for k in ``ks`` (default: one epoch) and the
        epoch's tail step will replay."""
        sizes = set()
        for k in (ks or (self.full_steps(),)):
            sizes.update(self.graph_plan(k, steps_per_graph))
        for n in sorted(sizes, reverse=True):
            if self.graph(n) is None:
                return
        if tail and self.tail_size() > 0:
            self.graph(1, tail=True)

    def stepper(self):
        """The native step executor (``csrc/bindings.cpp:LenetStepper``) for this engine's full
        steps: both kernels' argument blocks built once, ``run(k)`` enqueues 2k launches from
        C++.  None where a step is more than two launches (the all-reduce fallback)."""
        if self.comm and self.exch is None:
            return None
        # (the split-K fc scratch also next to the exchange, where the launcher does not use it)
        train, (name, update) = self.train_args(stage_next=True), self.update_launch("step", fc_split=True)
        key = launch_key((train, name, update))
        if self._stepper is None or self._stepper[0] != key:
            st = torch.classes.csed.LenetStepper()
            st.set_train(*train)
            (st.set_update_adam if name == "lenet_update_adam" else st.set_update)(*update)
            self._stepper = (key, st)
        return self._stepper[1]

    def step_plan(self, k: int, steps_per_graph: int = 16, use_graph: bool = True) -> list:
        """The launches that advance k full-batch steps from the current cursor, as a list of
        callables (graph replays, or native-executor runs where no graph applies), resolved up
        front so that a timed region holds nothing but the launches.

        Without graphs the native executor launches the steps from C++ (eager Python launches
        only where a step is more than two kernels).  Runs of at most ``self.native_max`` steps
        (``CSED_NATIVE_STEPS``, default 0) also take the executor instead of a graph replay:
        measured, graphs win even at 20 steps -- a replay's ~10 us setup is paid back by shorter
        gaps between its kernels (``profiles/bench_r2.md``, "Native step executor")."""
        if k <= 0:
            return []
        if not use_graph or self.capture_comm_ok is False or k <= self.native_max:
            st = self.stepper()
            return [self.step] * k if st is None else [lambda: st.run(k)]
        plan = []
        for n in self.graph_plan(k, steps_per_graph):
            g = self.graph(n)
            plan += [self.step] * n if g is None else [g.replay]
        return plan

    def run_steps(self, k: int, steps_per_graph: int = 16, use_graph: bool = True) -> None:
        """Advance k full-batch steps from the current cursor."""
        for launch in self.step_plan(k, steps_per_graph, use_graph):
            launch()

    def train_epoch(self, order: torch.Tensor, steps_per_graph: int = 16, use_graph: bool = True) -> None:
        self.set_epoch_order(order)
        self.run_steps(self.full_steps(), steps_per_graph, use_graph)
        self.last_partial_step(use_graph)

    # ---------------------------------------------------------------- metrics
    def take_loss(self) -> tuple[float, float]:
        """(sum of per-sample train NLL, correct count) since the last call (one host sync)."""
        v = self.loss_acc.tolist()
        self.loss_acc.zero_()
        return v[0], v[1]

    def _device_data(self, data: MNISTData) -> tuple[MNISTData, torch.Tensor]:
        """(``data`` on this engine's device, arange(len)), uploaded once per dataset object:
        evaluation runs every epoch and its 10k test images must not be re-copied each time."""
        hit = self._eval_cache.get(id(data))
        if hit is None or hit[0] is not data:
            dev = data if data.images.device == self.device else data.to(self.device)
            hit = (data, dev, _native.arange(len(data), self.device))
            self._eval_cache = {id(data): hit}
        return hit[1], hit[2]

    def _eval_weights(self, ema: bool) -> tuple[torch.Tensor, torch.Tensor]:
        """(weight image, fp32 parameters) an evaluation reads: the engine's own, or (``ema``) the moving
        average and its image, packed here from the average's current values (csed::lenet_pack)."""
        if not ema:
            return self.wimg, self.flat.data
        if self.ema is None:
            raise RuntimeError("no moving average is kept (set_ema)")
        if self._ema_wimg is None:  # (zero-initialised like wimg: the images' padding stays zero)
            self._ema_wimg = _native.zeros(lenet_layout().wimg_elems, torch.int16, self.device)
        torch.ops.csed.lenet_pack(self.ema, self._ema_wimg, self.mfma)
        return self._ema_wimg, self.ema

    @torch.no_grad()
    def evaluate(self, test: MNISTData, order: torch.Tensor | None = None, ema: bool = False) -> tuple[float, int]:
        """Forward-only pass over ``test``: (summed NLL, correct).  No dropout.  ``ema``: of the averaged
        parameters (set_ema) instead of the current ones."""
        test, ar = self._device_data(test)
        n = len(test)
        order = ar if order is None else order.to(self.device)
        nparts = min(n, 256)
        wimg, params = self._eval_weights(ema)
        torch.ops.csed.lenet_eval(test.images, test.labels, order, n, wimg, params, MNIST_MEAN,
                                  MNIST_STD, self.eval_parts, None, self.mfma)
        # (the 256 partial pairs summed on the host, in fixed order: a device reduction would be a
        # torch kernel whose code object loads at its first launch -- inside epoch 0)
        parts = self.eval_parts[: 2 * nparts].cpu().view(nparts, 2).double().sum(0).tolist()
        return parts[0], int(round(parts[1]))

    @torch.no_grad()
    def eval_logp(self, test: MNISTData, ema: bool = False) -> torch.Tensor:
        test, ar = self._device_data(test)
        n = len(test)
        out = torch.empty(n, 10, device=self.device)
        wimg, params = self._eval_weights(ema)
        torch.ops.csed.lenet_eval(test.images, test.labels, ar, n, wimg, params, MNIST_MEAN, MNIST_STD,
                                  self.eval_parts, out, self.mfma)
        return out

    # ------------------------------------------------------------ optimizer io
    def _adam_state_dict(self) -> dict:
        """What torch.optim.Adam / AdamW (amsgrad=False) of this torch return: per parameter the step number
        (a float32 scalar, theirs) and both moments, empty before the first step; one group."""
        state = {}
        t = int(self.step_count.item())
        if t > 0:
            for i in range(len(self.flat.params)):
                state[i] = {"step": torch.tensor(float(t), dtype=torch.float32),
                            "exp_avg": self.flat.view(self.momentum_buf, i).detach().cpu().clone(),
                            "exp_avg_sq": self.flat.view(self.adam_v, i).detach().cpu().clone()}
        lr = self.lr if self.lr_schedule is None else self.lr_schedule.current_lr()
        group = {"lr": lr, "betas": self.betas, "eps": self.eps, "weight_decay": self.weight_decay,
                 "amsgrad": False, "maximize": False, "foreach": None, "capturable": False,
                 "differentiable": False, "fused": None, "decoupled_weight_decay": self.optimizer == "adamw",
                 "params": list(range(len(self.flat.params)))}
        return {"state": state, "param_groups": [group]}

    def _load_adam_state_dict(self, sd: dict) -> None:
        g = sd["param_groups"][0]
        if "betas" not in g:
            raise ValueError(f"this optimizer state is not Adam's (its group has {sorted(g)}): the engine trains "
                             f"with {self.optimizer}")
        if bool(g.get("decoupled_weight_decay", False)) != (self.optimizer == "adamw"):
            raise ValueError(f"this optimizer state is {'AdamW' if g.get('decoupled_weight_decay') else 'Adam'}'s, "
                             f"the engine trains with {self.optimizer}")
        if g.get("amsgrad"):
            raise ValueError("amsgrad optimizer states are not supported")
        self.momentum_buf.zero_()
        self.adam_v.zero_()
        t = 0
        for i in range(len(self.flat.params)):
            st = sd.get("state", {}).get(i)
            if st:
                self.flat.view(self.momentum_buf, i).copy_(st["exp_avg"])
                self.flat.view(self.adam_v, i).copy_(st["exp_avg_sq"])
                t = int(st["step"])
        self.step_count.fill_(t)  # (the bias corrections continue at the saved step)
        self.lr, self.betas, self.eps = float(g["lr"]), (float(g["betas"][0]), float(g["betas"][1])), float(g["eps"])
        self.weight_decay = float(g["weight_decay"])
        self.invalidate()

    def optimizer_state_dict(self) -> dict:
        """torch.optim.SGD-compatible state dict (ref results/optimizer.pth); under Adam / AdamW theirs."""
        if self.adam:
            return self._adam_state_dict()
        state = {}
        if int(self.step_count.item()) > 0 and self.momentum != 0:
            for i in range(len(self.flat.params)):
                state[i] = {"momentum_buffer": self.flat.view(self.momentum_buf, i).detach().cpu().clone()}
        lr = self.lr if self.lr_schedule is None else self.lr_schedule.current_lr()  # (as a torch scheduler leaves it)
        group = {"lr": lr, "momentum": self.momentum, "dampening": self.dampening,
                 "weight_decay": self.weight_decay, "nesterov": self.nesterov, "maximize": False,
                 "foreach": None, "differentiable": False, "fused": None,
                 "params": list(range(len(self.flat.params)))}
        return {"state": state, "param_groups": [group]}

    def load_optimizer_state_dict(self, sd: dict) -> None:
        if self.adam:
            return self._load_adam_state_dict(sd)
        have = False
        self.momentum_buf.zero_()
        for i in range(len(self.flat.params)):
            st = sd.get("state", {}).get(i)
            if st and st.get("momentum_buffer") is not None:
                self.flat.view(self.momentum_buf, i).copy_(st["momentum_buffer"])
                have = True
        self.step_count.fill_(1 if have else 0)
        g = sd["param_groups"][0]
        self.lr, self.momentum = float(g["lr"]), float(g["momentum"])
        self.invalidate()  # (what held the old lr / momentum is not replayed again)

    def set_lr_schedule(self, schedule) -> None:
        """Train at ``schedule``'s rates (optim.LRSchedule, moved to the engine's device) from its current
        position on, or at the constant ``self.lr`` again (None).  lenet_update then reads its step's
        table entry on the device and advances the position: the steps of one graph, or of one
        native-executor run, train at different rates.  Captured graphs and the executor's argument
        blocks hold the old rate or table: dropped, as in load_optimizer_state_dict."""
        self.lr_schedule = None if schedule is None else schedule.to(self.device)
        self.invalidate()

    def set_ema(self, decay: float | None) -> None:
        """Keep an exponential moving average of the parameters, ``e <- e + (1 - decay) * (p_new - e)`` in
        fp32, updated on the device by every launch that applies SGD (full and tail steps, at any world
        size: the summed gradient is the same on every rank, so are the averages), started at a copy of
        the current parameters.  None switches it off and frees the buffer.  Captured graphs and the
        executor's argument blocks hold the old buffer or none: dropped, as in set_lr_schedule."""
        if decay is None:
            self.ema, self.ema_decay, self._ema_wimg = None, 0.0, None
        else:
            if not 0.0 <= float(decay) < 1.0:
                raise ValueError(f"ema decay {decay}: expected 0 <= decay < 1")
            if self.ema is None:  # (the extension's own fill; the copy below is a device-to-device memcpy)
                self.ema = _native.zeros(self.flat.data.shape, torch.float32, self.device)
            self.ema.copy_(self.flat.data)
            self.ema_decay = float(decay)
        self.invalidate()

    def ema_state_dict(self) -> dict:
        """The averaged parameters under ``Net``'s parameter names (fp32 CPU tensors): loads into the
        reference ``Net`` with ``load_state_dict``."""
        if self.ema is None:
            raise RuntimeError("no moving average is kept (set_ema)")
        return {n: self.flat.view(self.ema, i).detach().cpu().clone()
                for i, (n, _) in enumerate(self.model.named_parameters())}

    def load_ema_state_dict(self, sd: dict) -> None:
        """Restore ``ema_state_dict()``'s values (EMA must be on: the decay is not part of the file)."""
        if self.ema is None:
            raise RuntimeError("no moving average is kept (set_ema)")
        for i, (n, _) in enumerate(self.model.named_parameters()):
            self.flat.view(self.ema, i).copy_(sd[n])

    def params_changed(self) -> None:
        """Call after writing the model parameters from outside (e.g. a checkpoint load)."""
        self.repack()

    # --------------------------------------------------------------- smoke
    @classmethod
    def smoke_instance(cls, device) -> "FusedLeNetTrainer":
        from ..data.mnist import synthetic_mnist

        torch.manual_seed(1)
        net = Net().to(device)
        data = synthetic_mnist(64, seed=3)
        return cls(net, data, lr=0.01, momentum=0.5, global_batch=16)

    def smoke_step(self) -> None:
        self.set_epoch_order(torch.arange(64))
        self.step()
        torch.cuda.synchronize(self.device)
        loss, _ = self.take_loss()
        if not math.isfinite(loss):
            raise RuntimeError("fused smoke step produced a non-finite loss")
