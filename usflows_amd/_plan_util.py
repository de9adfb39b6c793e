"""What engine.py and the two plan builders (engine_flat.py, engine_planes.py) share: a leaf module, it imports none of them."""
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


def affine_span(prims, k: int):
    """(fuse_post, is_last, primitives taken) of the affine primitive prims[k] in either builder: the multiplication of a
    ScaleTransform right behind an ``affine_fwd`` rides in that GEMM's epilogue (the block then takes two primitives), and the
    block that ends the list writes the plan's result in the natural layout"""
    n = len(prims)
    fuse_post = prims[k][0] == "affine_fwd" and k + 1 < n and prims[k + 1][0] == "scale_mul"
    taken = 2 if fuse_post else 1
    return fuse_post, k + taken == n, taken


def folded_bias(a: dict) -> torch.Tensor:
    """the folded bias c = -(Minv b) of an affine block's pack entry a, formed in fp64 on first use and kept as a["c"]:
    (y - b) @ Minv^T == y @ Minv^T + c keeps the bias out of the K loop's registers ("bias folding").  Launched where
    it stands -- it reads the prepared M^-1 and b only, so it may run in front of queued image jobs (the job that packs c leaves
    with the batch) -- and onto whatever tape the caller records: both builders run inside ``_build_plan``'s ``_pk_record``."""
    if "c" not in a:
        a["c"] = torch.empty(a["b"].shape, dtype=torch.float64, device=a["b"].device)
        _ext.matvec_f64(a["Minv"], a["b"].contiguous(), alpha=-1.0, out64=a["c"])
    return a["c"]
