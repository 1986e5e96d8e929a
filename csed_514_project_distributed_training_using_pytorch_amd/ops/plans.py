"""Which kernel form a GEMM launch takes: the struct the launcher itself dispatches on (csrc/launchers.h
``GemmPlan``), asked through ``csed::gemm_plan`` and ``csed::linear_bwd_plan`` with the tensors the op itself
would get (their shapes, dtypes, strides and alignment decide; nothing is read or launched)."""
from __future__ import annotations

from typing import NamedTuple

import torch

from . import _native

SCALAR, K_CONTIG, R_CONTIG = 0, 1, 2  # GemmPlan.a_mode / b_mode


class GemmPlan(NamedTuple):
    """``csed::GemmPlan``, in its order."""
    small: int
    splits: int
    tiles: int
    grid_x: int
    grid_y: int
    a_mode: int
    b_mode: int


class LinearBwdPlan(NamedTuple):
    """``linear_bwd``: both GEMMs in one launch of the pair kernel, and each GEMM's plan (dx first, then dw)."""
    pairable: int
    gemms: tuple


def _code(dtype: torch.dtype) -> int:
    return _native.MFMA_CODE[dtype]


def gemm_plan(A, B, C, compute: torch.dtype, gate=None, rowsum=None) -> GemmPlan:
    return GemmPlan(*(int(v) for v in _native.ops().gemm_plan(A, B, C, gate, _code(compute), rowsum)))


def linear_bwd_plan(dy, x, w, compute: torch.dtype, gate=None, dx=None, dw=None, db=None) -> LinearBwdPlan:
    v = [int(i) for i in _native.ops().linear_bwd_plan(dy, x, w, gate, dx, dw, db, _code(compute))]
    n = len(GemmPlan._fields)
    return LinearBwdPlan(v[0], tuple(GemmPlan(*v[1 + i:1 + i + n]) for i in range(0, len(v) - 1, n)))
