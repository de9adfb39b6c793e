"""What engine.py and engine_planes.py both need (a leaf module: it imports neither)."""
from __future__ import annotations

import torch

from . import _ext


class EngineUnsupported(Exception):
    """The layer list contains something the fused device path cannot express."""


def _round_up(n: int, m: int) -> int:
    return (n + m - 1) // m * m


def _refreshed(shape, dtype, device, fn) -> torch.Tensor:
    """persistent tensor filled by fn(out) now and again on every replay of the pack tape"""
    out = torch.empty(shape, dtype=dtype, device=device)
    _ext.host_op(lambda: fn(out))
    return out


def _image_triple(W: torch.Tensor):
    """(pointer, leading dimension, plane stride) of a weight image [planes, rows, cols]"""
    return W.data_ptr(), W.shape[2], W.shape[1] * W.shape[2]


def arange_padded(n_valid: int, n_total: int) -> torch.Tensor:
    """host selector [0 .. n_valid-1, -1, -1, ...] of length n_total (-1: a zero row / column of the image)"""
    t = torch.full((n_total,), -1, dtype=torch.long)
    t[:n_valid] = torch.arange(n_valid)
    return t


def kperm(n_valid: int, Hp: int, device) -> torch.Tensor:
    """int32 device selector of a hidden (K) axis of Hp columns in the accumulator order of the fused coupling kernel
    (positions >= n_valid: -1)"""
    g, j = torch.arange(4)[:, None], torch.arange(8)[None, :]
    within = torch.where(j < 4, 4 * g + j, 16 + 4 * g + (j - 4)).reshape(-1)          # [32]
    perm = (torch.arange(0, Hp, 32)[:, None] + within[None, :]).reshape(-1)
    return torch.where(perm < n_valid, perm, torch.full_like(perm, -1)).to(device=device, dtype=torch.int32)
