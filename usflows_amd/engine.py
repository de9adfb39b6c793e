"""Device engine: compiles a list of USFlows layers into a chain of HIP kernel launches.

What it does, per flow (see DESIGN.md for the rationale):

* **parameter pack** (cached per parameter version): for every affine block the dense ``M``,
  ``M^-1`` (triangular solves in fp64 on the device, rounded once to fp32), bias and
  ``sum log|diag U|``; for every coupling the mask-aware slices of the conditioner weights.  The
  reference re-derives all of this on every ``log_prob`` call (transforms.py:1289-1293, 795-809).
* **segment layout**: between layers the activation matrix is stored ``[mask==0 features |
  mask==1 features]`` (each segment padded to 4 floats), so a coupling layer's conditioning half
  and transformed half are *contiguous* column ranges -- no strided gathers, and the ``x*mask`` /
  ``(1-mask)*NN`` zeros of the reference are never multiplied.  The permutation is folded into
  the rows/columns of the neighbouring affine matrices at pack time, i.e. it is free.
* **op list**: fused linear ops (``usf_linear_f32``: scale / bias prologue + GEMM + bias /
  LeakyReLU / residual / scale epilogue), optionally the fused coupling kernel, then the base
  density tail (``usf_base_logprob_f32``).  The whole list is launched by ONE ``usf_run_ops``
  call on torch's current stream.

This module holds the analysis, the layouts, the affine blocks' pack, the workspace, the plan cache and the execution; the two
builders that lay out an op list are mixins: engine_flat.py (fp32 rows between layers) and engine_planes.py (planes).

No arithmetic of the device path is done by torch ops, except the (cached, batch-independent)
parameter prep and the O(B) finishing formula of the radial density.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Dict, List, Optional, Sequence, Tuple

import torch
from torch import nn

from . import _ext
from . import transforms as T
from .config import config
from ._plan_util import EngineUnsupported, _refreshed, _round_up, folded_bias  # noqa: F401  -- EngineUnsupported: re-exported
from .networks import ConditionalDenseNN, ConvNet, DenseNN
from .engine_flat import FlatPlanMixin
from .engine_planes import PlanesPlanMixin


def _activation_of(f) -> Optional[Tuple[int, float]]:
    if isinstance(f, nn.LeakyReLU):
        return _ext.ACT_LEAKY_RELU, float(f.negative_slope)
    if isinstance(f, nn.ReLU):
        return _ext.ACT_LEAKY_RELU, 0.0
    return None


def conditioner_supported(cond: nn.Module) -> bool:
    if getattr(cond, "consumes_context", False):
        return False                     # (CondConvNet: the flat plan's context columns feed ConditionalDenseNN's layers[1] only)
    if isinstance(cond, ConditionalDenseNN):
        # the context columns of the workspace: one (the fused kernels' scalar form) up to VCTX_MAX (their vector form)
        return 1 <= cond.context_dim <= _ext.VCTX_MAX and _activation_of(cond.f) is not None
    if isinstance(cond, DenseNN):
        return cond.count_params == 1 and _activation_of(cond.f) is not None
    if isinstance(cond, ConvNet):        # vector path: plain chain of Linears, or GatedMLP / LayerNormVector blocks
        return cond.is_vector and _activation_of(cond.f) is not None     # (spatial path: image-shaped flows, the layer loop)
    return False


def conditioner_layers(cond: nn.Module):
    """(first, context layer | None, hidden layers, last) of a DenseNN's / ConditionalDenseNN's ``layers``: the context
    layer ([h0, context_dim]) sits behind the first"""
    lin = list(cond.layers)
    if isinstance(cond, ConditionalDenseNN):
        return lin[0], lin[1], lin[2:-1], lin[-1]
    return lin[0], None, lin[1:-1], lin[-1]


@dataclass
class _Step:
    kind: str            # 'scale' | 'affine' | 'coupling'
    module: nn.Module    # ScaleTransform | AffineTransform block | MaskedCoupling
    inverted: bool       # wrapped in InverseTransform


class _MergedAffine:
    """Stand-in block for a run of consecutive affine steps of one direction (inference plans only): with
    ``affine_conjugation`` every coupling is followed by block_i^-1 and block_(i+1), two dense D x D maps with nothing
    in between -- applied as ONE map y = (W2 W1) x + (W2 c1 + c2) composed in fp64 at pack time (half the affine GEMMs
    of such a flow; the reference applies them one by one).  ``pk["affine"][id(self)]`` holds the composite as the M / b
    of an ``affine_fwd`` step."""

    def __init__(self, parts):
        self.parts = parts          # [(prim, block)] in application order


def _analyze(layers: Sequence[nn.Module]) -> List[_Step]:
    steps = []
    for l in layers:
        inv = False
        while isinstance(l, T.InverseTransform):
            inv = not inv
            l = l.transform
        if isinstance(l, T.ScaleTransform) and l.scale.dim() == 1:
            steps.append(_Step("scale", l, inv))
        elif isinstance(l, T.BlockAffineTransform):
            steps.append(_Step("affine", l.block_transform, inv))
        elif isinstance(l, (T.LUTransform, T.HouseholderTransform, T.SequentialAffineTransform)):
            steps.append(_Step("affine", l, inv))
        elif isinstance(l, T.MaskedCoupling) and l.mask.dim() == 2 and conditioner_supported(l.conditioner):
            steps.append(_Step("coupling", l, inv))
        else:
            raise EngineUnsupported(f"layer {type(l).__name__} has no fused device form")
    if not steps:
        raise EngineUnsupported("empty layer list")
    if len(context_dims(steps)) > 1:
        raise EngineUnsupported("couplings of one flow disagree on context_dim (one context workspace per plan)")
    return steps


def context_dims(steps) -> set:
    """the context widths of a step list's ConditionalDenseNN conditioners"""
    return {int(s.module.conditioner.context_dim) for s in steps
            if s.kind == "coupling" and isinstance(s.module.conditioner, ConditionalDenseNN)}


# ---------------------------------------------------------------------------------------------
# fp64 parameter prep: batched HIP kernels (usf_prep.hip), cached per parameter version
# ---------------------------------------------------------------------------------------------
_copied_params = [0]      # bumped whenever _param had to COPY a parameter (a pack built from copies cannot be replayed)


def _param(t: torch.Tensor, device=None) -> torch.Tensor:
    """fp32 contiguous device view of a parameter (its own storage when it already is one)"""
    src = t
    t = t.detach()
    if device is not None and t.device != torch.device(device):
        t = t.to(device)
    if t.dtype != torch.float32:
        t = t.float()
    t = t if t.is_contiguous() else t.contiguous()
    if t.data_ptr() != src.data_ptr():
        _copied_params[0] += 1
    return t


class LogDet:
    """Sum of the layers' log|det J| (parameter-only for these flows: flows.py:236-245).  ``neg_dev`` is a persistent
    fp64 device scalar holding MINUS the total (what log_prob adds); kernels take its pointer
    (``usf_base_logprob_f32(logdet_dev=...)``), torch expressions the tensor.  ``float(obj)`` is the total as a Python
    float -- the one host read-back, done on demand and cached until the next refresh."""
    __slots__ = ("neg_dev", "_val")

    def __init__(self, neg_dev):
        self.neg_dev, self._val = neg_dev, (0.0 if neg_dev is None else None)

    def refresh(self, total: torch.Tensor) -> None:
        torch.neg(total, out=self.neg_dev)
        self._val = None

    def __float__(self) -> float:
        if self._val is None:
            self._val = -float(self.neg_dev.item())
        return self._val

    def neg32(self, device) -> torch.Tensor:
        """-total as a 0-dim fp32 tensor on ``device`` (for torch-side sums)"""
        if self.neg_dev is None:
            return torch.zeros((), dtype=torch.float32, device=device)
        return self.neg_dev.to(torch.float32)


_PERM_CONST: dict = {}      # FlowEngine._perm_vec: constants of a (layout index, padding) pair


def prepare_affine_blocks(blocks: Sequence[nn.Module], device=None, keep_factors: bool = False) -> Dict[int, dict]:
    """``id(block) -> dict(M, Minv, b, ladj)`` (fp64 device tensors) for LUTransform / HouseholderTransform /
    SequentialAffineTransform blocks, following the reference's definitions (transforms.py:1271-1320, 795-809,
    1457-1476).  All LU blocks of the flow go through ONE batched ``usf_lu_prepare_f64`` call (chunked only to
    bound the fp64 scratch at large D).  Every result lives in a tensor of its own that a replay of the recording
    tape (``_ext.Tape``) refills in place: pointers handed to plans stay valid across optimiser steps."""
    lus: Dict[int, nn.Module] = {}
    hhs: Dict[int, nn.Module] = {}

    def visit(b):
        if isinstance(b, T.LUTransform):
            lus.setdefault(id(b), b)
        elif isinstance(b, T.HouseholderTransform):
            hhs.setdefault(id(b), b)
        elif isinstance(b, T.SequentialAffineTransform):
            for t in b.transforms:
                visit(t)
        else:
            raise EngineUnsupported(type(b).__name__)

    for b in blocks:
        visit(b)
    res: Dict[int, dict] = {}
    lu_list = list(lus.values())
    chunks = []
    if lu_list:
        D = int(lu_list[0].dim)
        chunk = max(1, min(len(lu_list), int(8e9 // (64 * D * D))))       # 8 fp64 [D,D] arrays per block in flight
        for c0 in range(0, len(lu_list), chunk):
            part = lu_list[c0: c0 + chunk]
            out = _ext.lu_prepare([_param(l.L_raw, device) for l in part], [_param(l.U_raw, device) for l in part],
                                  keep_factors=keep_factors)
            dev = out["ladj"].device
            bias = [_param(l.bias_vector, device) for l in part]
            b64 = _refreshed((len(part), D), torch.float64, dev,
                             lambda o, bias=bias: o.copy_(torch.stack(bias)))       # (one gather + one converting copy, not one per block)
            chunks.append(dict(lus=part, out=out, b=b64))
            # bias folding, (y - b) Minv^T == y Minv^T + c: c = -(Minv b) of ALL blocks in one batched launch (it was one
            # usf_matvec_f64 per block on the pack's tape: 32 launches of every small-batch training step)
            c64 = torch.empty(len(part), D, dtype=torch.float64, device=dev)
            _ext.gemm_f64(b64, out["Minv"], c64, batch=len(part), M=1, N=D, K=D, lda=D, ldb=D, ldc=D, strideA=D, strideB=D * D,
                          strideC=D, transB=True, alpha=-1.0)
            for j, l in enumerate(part):
                r = dict(M=out["M"][j], Minv=out["Minv"][j], b=b64[j], c=c64[j], ladj=out["ladj"][j])
                if keep_factors:
                    r.update(L=out["tri"][2 * j], Ut=out["tri"][2 * j + 1], Linv=out["tri_inv"][2 * j],
                             Uinv_t=out["tri_inv"][2 * j + 1])
                res[id(l)] = r
    hh_list = list(hhs.values())
    if hh_list:
        D = int(hh_list[0].dim)
        dev = torch.device(device) if device is not None else hh_list[0].w_0.device
        Hs = torch.empty(len(hh_list), D, D, dtype=torch.float64, device=dev)     # one stack: batched composition below
        HsT = torch.empty(len(hh_list), D, D, dtype=torch.float64, device=dev)
        zero = torch.zeros(D, dtype=torch.float64, device=dev)
        for i, h in enumerate(hh_list):
            _ext.householder(_param(h.w_0, device), _param(h.vk_householder, device), out=Hs[i])
        _ext.host_op(lambda: HsT.copy_(Hs.transpose(1, 2)))                       # (after the launches above)
        for i, h in enumerate(hh_list):
            res[id(h)] = dict(M=Hs[i], Minv=HsT[i], b=zero, ladj=zero.sum(), row=i)
    seq = [b for b in blocks if isinstance(b, T.SequentialAffineTransform) and id(b) not in res]
    # the USFlow constructor's block: Sequential([LU, Householder]) for every coupling block.  When the LU factors are
    # rows first .. first+m-1 of one prepare chunk and the Householder factors rows 0 .. m-1 of their stack, the
    # composition (transforms.py:1457-1476) is three batched launches instead of three per block
    batched = False
    if (len(seq) > 1 and len(chunks) == 1 and all(len(b.transforms) == 2 and isinstance(b.transforms[0], T.LUTransform)
                                                  and isinstance(b.transforms[1], T.HouseholderTransform) for b in seq)):
        lu_row = {id(l): j for j, l in enumerate(chunks[0]["lus"])}
        rows = [lu_row[id(b.transforms[0])] for b in seq]
        hrows = [res[id(b.transforms[1])]["row"] for b in seq]
        m = len(seq)
        if rows == list(range(rows[0], rows[0] + m)) and hrows == list(range(m)):
            out, D = chunks[0]["out"], int(seq[0].dim)
            DD, r0 = D * D, rows[0]
            f64 = lambda *shape: torch.empty(*shape, dtype=torch.float64, device=Hs.device)
            Mt, Mit, bt = f64(m, D, D), f64(m, D, D), f64(m, D)
            bat = dict(batch=m, M=D, N=D, K=D, lda=D, ldb=D, ldc=D, strideA=DD, strideB=DD, strideC=DD)
            _ext.gemm_f64(out["M"], Hs, Mt, a_off=r0 * DD, **bat)                          # M_lu H
            _ext.gemm_f64(Hs, out["Minv"], Mit, transA=True, b_off=r0 * DD, **bat)         # H^T M_lu^-1
            _ext.gemm_f64(chunks[0]["b"], Hs, bt, batch=m, M=1, N=D, K=D, lda=D, ldb=D, ldc=D, strideA=D, strideB=DD,
                          strideC=D, a_off=r0 * D)                                         # b_lu H
            ct = f64(m, D)
            _ext.gemm_f64(bt, Mit, ct, batch=m, M=1, N=D, K=D, lda=D, ldb=D, ldc=D, strideA=D, strideB=DD, strideC=D, transB=True,
                          alpha=-1.0)                                                      # c = -(Minv b), as for the LU blocks
            for i, b in enumerate(seq):
                res[id(b)] = dict(M=Mt[i], Minv=Mit[i], b=bt[i], c=ct[i], ladj=out["ladj"][r0 + i])  # (Householder: ladj 0)
            batched = True
    for b in (seq if not batched else []):
        if True:                                                                  # general composition, block by block
            parts = [res[id(t)] for t in b.transforms]
            M, Minv, bias = parts[0]["M"], parts[0]["Minv"], parts[0]["b"]      # eye @ M_1 == M_1 exactly
            ladj = parts[0]["ladj"]
            for p_ in parts[1:]:                                                  # :1457-1462, :1471-1476
                M = _ext.matmul_f64(M, p_["M"])
                bm = _ext.matmul_f64(bias.reshape(1, -1), p_["M"])
                bias = _refreshed(tuple(p_["b"].shape), torch.float64, bm.device,
                                  lambda o, bm=bm, pb=p_["b"]: torch.add(bm.reshape(-1), pb, out=o))
                Minv = _ext.matmul_f64(p_["Minv"], Minv)                          # :1464-1469 (reverse order)
                ladj = _refreshed((), torch.float64, bm.device,
                                  lambda o, a=ladj, c=p_["ladj"]: torch.add(a, c, out=o))
            res[id(b)] = dict(M=M, Minv=Minv, b=bias, ladj=ladj)
            if len(parts) == 1 and "c" in parts[0]:
                res[id(b)]["c"] = parts[0]["c"]          # Sequential([LU]): the block IS its LU factor, folded bias included
    res["__chunks__"] = chunks
    return res


class FlowEngine(FlatPlanMixin, PlanesPlanMixin):
    """Compiled device form of ``layers`` (a whole ``Flow`` or a single layer)."""

    def __init__(self, layers: Sequence[nn.Module]):
        self.steps = _analyze(layers)
        self.D = self._infer_dim()
        self._pack = None
        self._pack_key = None
        self._plans: Dict[tuple, dict] = {}
        self._ws: Dict[tuple, Dict[str, torch.Tensor]] = {}
        # Consecutive affine steps of an inference plan run as ONE composed map (_MergedAffine) -- with affine_conjugation
        # (every live configuration of the reference) that halves the D x D GEMMs.  The reference applies the maps one
        # by one in fp32, and on badly conditioned (default-initialised) blocks the composite rounds differently -- golden
        # init_d7_k2_hh1_conj_laplace: relative log_prob error 4e-6 one by one, 1.0e-5 composed (well-conditioned
        # flows: unchanged, 5e-8 .. 1.5e-7).  merge_affine = "auto" (default): every run of layers is composed only if a
        # pack-time probe says the composite is as accurate as the run applied layer by layer (_merge_guard); True
        # (USFLOWS_AMD_MERGE_AFFINE=1): always; False (=0): never.
        self.merge_affine = config.merge_affine
        self.merge_guard_log: List[tuple] = []   # (accepted, element-wise deviation, L1-norm deviation) of composed vs layer-by-layer, per probe
        self._virtual: List[_Step] = []          # merged steps, addressed as step index len(self.steps) + n
        self._virtual_ix: Dict[tuple, int] = {}
        self.launch_count = 0          # number of usf_run_ops calls (tests assert the HIP path ran)
        self.op_timing = None          # set to a list to record (tag, start_event, end_event) per op (bench.py)
        self.use_fused_coupling = True
        self.fused_min_rows = 14336    # measured cross-over on MI355X at D=784, hidden 256 (bench.py --fused-min-rows sweep:
        #                                fused / unfused ms per step: 8192 4.79 / 3.98, 12288 5.06 / 5.05, 16384 6.45 / 6.66, 20480 7.54 / 8.43)
        # "bf16x3": the GEMMs run on the bf16 matrix cores with a 3-way residual split of both operands (24 significant
        # bits, six MFMAs per product); "f16x2": the planes pipeline uses two fp16 planes per operand
        # (22 significant bits, three MFMAs per product, range-guarded with a bf16x3 redo; everything outside the planes
        # pipeline as "bf16x3"); "f32": exact-f32 MFMA everywhere (USFLOWS_AMD_GEMM=... or engine.gemm_mode = ...)
        self.gemm_mode = config.gemm_mode
        # True: the pack also keeps L, U^T, L^-1, U^-T of every LU block (fp64) -- the training backward's operands
        self.keep_factors = False
        # USFLOWS_AMD_GRAPH=1: batches up to graph_max_rows replay their launch list as one hipGraph.  Off by default:
        # measured on MI355X / ROCm 7.2 the replay is no faster than the C-side launch loop of usf_run_ops (cfg2,
        # B = 100: 1.22 ms either way) -- the ~7 us between two dependent dispatches is not host time
        # planes pipeline: from planes_min_rows rows, inference plans in bf16x3 mode keep the activations
        # between layers as pre-split bf16 planes in MFMA-operand order (usf_planes.hip); USFLOWS_AMD_PLANES=0 disables
        self._f16_overflow = False      # set while a pass is being redone in bf16x3 because fp16 planes overflowed
        self.f16_fallbacks = 0          # number of such passes (tests / diagnostics)
        # use_planes: None = automatic, True / False = forced (USFLOWS_AMD_PLANES=1 / 0).  Automatic: "f16x2" mode from
        # planes_min_rows rows; "bf16x3" mode from planes_min_rows_bf16x3 rows (measured on MI355X, cfg2, ms per step
        # planes / fp32-activation kernels, round 3, same box: 16384 6.77 / 6.55-6.78, 24576 7.48 / 7.75, 32768 9.71 / 9.91
        # -- the per-rank shard of the 8-GPU configuration cfg3 --, 40960 14.05 / 14.30, 65536 18.8 / 19.2),
        # or from planes_min_rows when a conditioner is too wide / deep for the fused coupling kernels (cfg4, hidden 1024:
        # 176.6 vs 215.8 ms at 32768 rows)
        self.use_planes = config.planes
        self.planes_min_rows = int(config.planes_min_rows)
        self.planes_min_rows_bf16x3 = 24576
        # inference plans: an affine layer hands the transformed half of its output to the fused coupling behind it as fp32
        # beside the planes (usf_gemm_planes_side / usf_coupling_planes_side).  Knob planes_side_f32 = 0 builds the
        # launch list without it (the A/B arm).  From planes_side_min_rows rows: the smallest batch at which a planes plan is
        # chosen automatically -- below it (forced plans) the list stays the plain one, which is all that was measured there
        self.planes_side_f32 = bool(config.planes_side_f32)
        self.planes_side_min_rows = 8192
        # training on the planes pipeline (round 5): the forward keeps every layer's planes buffer and the conditioners' hidden
        # activations as planes, the backward runs on usf_gemm_planes_bf16x3 / usf_coupling_planes (gate mode) /
        # usf_wgrad_blocked_f32.  USFLOWS_AMD_TRAIN_PLANES=0 keeps the fp32-row path of rounds 3 / 4.
        self.use_train_planes = config.train_planes
        self.train_planes_min_rows = 16384
        # a context on the planes plans (usf_coupling_planes_ctx): smallest batch at which a flow WITH a context
        # takes the planes plan in automatic mode (use_planes = None) resp. the planes training step, on top of the conditions
        # above.  None = never: the context form has not been timed against the fp32-activation plan / the fp32-row path, which
        # serve these flows as before, and goes on by default only behind a measured cross-over (tools/bench_ctx_planes.py).
        # use_planes = True forces the inference plans as for every flow; training has no forced mode, so set the second knob
        self.ctx_planes_min_rows = None
        self.train_ctx_planes_min_rows = None
        self.use_graphs = bool(config.engine_graph)
        self.graph_max_rows = 1024
        self._layout_from_masks()

    # ---- static structure ---------------------------------------------------------------------
    def _infer_dim(self) -> int:
        for s in self.steps:
            if s.kind == "scale":
                return int(s.module.scale.shape[0])
            if s.kind == "affine":
                return int(s.module.dim)
            if s.kind == "coupling":
                return int(s.module.mask.shape[-1])
        raise EngineUnsupported("cannot infer dimension")

    def _layout_from_masks(self):
        D = self.D
        base = None
        self._flip = {}
        for i, s in enumerate(self.steps):
            if s.kind != "coupling":
                continue
            m = s.module.mask.detach().flatten().cpu()
            if m.numel() != D or not bool(((m == 0) | (m == 1)).all()):
                raise EngineUnsupported("coupling mask must be a 0/1 vector of length D")
            if base is None:
                base = m
            if torch.equal(m, base):
                self._flip[i] = False
            elif torch.equal(m, 1 - base):
                self._flip[i] = True
            else:
                raise EngineUnsupported("coupling masks must alternate between m and 1-m")
        if base is None:
            idx0 = torch.arange(D)
            idx1 = torch.zeros(0, dtype=torch.long)
        else:
            idx0 = torch.nonzero(base == 0).flatten()
            idx1 = torch.nonzero(base == 1).flatten()
        self.n0, self.n1 = int(idx0.numel()), int(idx1.numel())
        self.n0a, self.n1a = _round_up(self.n0, 4), _round_up(self.n1, 4)
        self.LD = max(self.n0a + self.n1a, 4)
        seg = torch.full((self.LD,), -1, dtype=torch.long)
        seg[: self.n0] = idx0
        seg[self.n0a: self.n0a + self.n1] = idx1
        self.seg_idx = seg
        self.LDn = _round_up(D, 4)
        nat = torch.full((self.LDn,), -1, dtype=torch.long)
        nat[:D] = torch.arange(D)
        self.nat_idx = nat
        # the same two layouts padded to whole 32-feature blocks (planes pipeline, usf_planes.hip)
        self.LDp, self.LDnp = _round_up(self.LD, 32), _round_up(D, 32)
        self.segp_idx = torch.full((self.LDp,), -1, dtype=torch.long)
        self.segp_idx[: self.LD] = seg
        self.natp_idx = torch.full((self.LDnp,), -1, dtype=torch.long)
        self.natp_idx[:D] = torch.arange(D)
        self.ctx_dim = max(context_dims(self.steps), default=1)      # context columns of the workspace (_analyze: one width per flow)
        self.hmax = 4
        self._general_cond = False       # a conditioner with gate / layer-norm blocks: chain of ops, no fused kernel
        for s in self.steps:
            if s.kind == "coupling":
                cond = s.module.conditioner
                widths = cond.c_hidden if isinstance(cond, ConvNet) else cond.hidden_dims
                self.hmax = max(self.hmax, max(_round_up(int(h), 4) for h in widths))
                self._general_cond = self._general_cond or (isinstance(cond, ConvNet) and not cond.is_plain_mlp())

    def _params(self):
        seen, out = set(), []
        for s in self.steps:
            for p in s.module.parameters():
                if id(p) not in seen:
                    seen.add(id(p))
                    out.append(p)
        return out

    # ---- parameter pack -----------------------------------------------------------------------
    def _version_key(self, device):
        return (str(device),) + tuple((p.data_ptr(), p._version) for p in self._params())

    def refresh(self):
        """Drop the cached parameter pack (it is also rebuilt automatically when a parameter's
        version counter or storage changes)."""
        self._pack, self._pack_key = None, None
        self._plans.clear()

    def _idx(self, layout: str) -> torch.Tensor:
        return {"seg": self.seg_idx, "nat": self.nat_idx, "segp": self.segp_idx, "natp": self.natp_idx}[layout]

    @staticmethod
    def _perm_mat(mat64: torch.Tensor, out_idx: torch.Tensor, in_idx: torch.Tensor) -> torch.Tensor:
        dev = mat64.device
        oi, ii = out_idx.to(dev), in_idx.to(dev)
        W = torch.zeros(oi.numel(), ii.numel(), dtype=torch.float64, device=dev)
        ro, ci = torch.nonzero(oi >= 0).flatten(), torch.nonzero(ii >= 0).flatten()
        W[ro[:, None], ci[None, :]] = mat64[oi[ro][:, None], ii[ci][None, :]]
        return W.float().contiguous()

    @staticmethod
    def _perm_vec(v64: torch.Tensor, idx: torch.Tensor, pad: float) -> torch.Tensor:
        # (no boolean-mask indexing, no host index tensor: both would synchronise the host on every pack refresh,
        # i.e. on every optimiser step.  What depends on the layout alone -- the gather index, the keep mask, the padding --
        # is built once per index tensor: a refresh is a gather, one fused multiply-add and the rounding, not eight launches)
        idx = idx.to(v64.device)
        key = (idx.data_ptr(), float(pad), str(v64.device))
        ent = _PERM_CONST.get(key)
        if ent is None or ent[0] is not idx:
            valid = idx >= 0
            ent = _PERM_CONST[key] = (idx, idx.clamp(min=0).long(), valid.to(torch.float64),
                                      torch.where(valid, 0.0, float(pad)).to(torch.float64))
            if len(_PERM_CONST) > 256:
                _PERM_CONST.clear()
        _, gidx, keep, padv = ent
        return torch.addcmul(padv, v64[gidx], keep).float()

    def _ptr_key(self, device):
        return (str(device), self.keep_factors) + tuple(p.data_ptr() for p in self._params())

    def pack(self, device) -> dict:
        key = self._version_key(device)
        pk = self._pack
        if pk is not None and key == self._pack_key and (pk["has_factors"] or not self.keep_factors):
            return pk
        if (pk is not None and _ext.TAPES_ENABLED and pk["replayable"] and torch.device(device).type == "cuda"
                and pk["ptr_key"] == self._ptr_key(device) and pk["tape"].stream == _ext.current_stream(device)):
            # same parameter storage, new values (an optimiser step): refill every prepared tensor in place by
            # replaying the recorded launches -- plans and their device pointers stay valid
            with torch.no_grad():
                _ext.replay(pk["tape"])
                pk["ladj_total"] = self._ladj_total(pk)
            self._pack_key = key
            pk["replays"] = pk.get("replays", 0) + 1
            if pk["replays"] % 256 == 0:
                pk.pop("auto_merge", None)          # training moves the parameters: probe the composed plans again
            return pk
        pk = {"affine": {}, "coupling": {}, "scale": {}, "mats": {}, "vecs": {}, "has_factors": self.keep_factors,
              "tape": _ext.Tape(), "ptr_key": self._ptr_key(device), "ladj_terms": []}
        pk["tape"].stream = _ext.current_stream(device) if torch.device(device).type == "cuda" else None
        copies0 = _copied_params[0]
        convnet = False
        with torch.no_grad(), _ext.record(pk["tape"]):
            blocks, seen = [], set()
            for s in self.steps:
                if s.kind == "affine" and id(s.module) not in seen:
                    seen.add(id(s.module))
                    blocks.append(s.module)
            prepared = prepare_affine_blocks(blocks, device, keep_factors=self.keep_factors)
            pk["affine_parts"] = prepared          # also the LU / Householder factors inside Sequential blocks
            for b_ in blocks:
                pk["affine"][id(b_)] = prepared[id(b_)]
            for i, s in enumerate(self.steps):
                if s.kind == "affine":
                    pk["ladj_terms"].append((-1.0 if s.inverted else 1.0, pk["affine"][id(s.module)]["ladj"]))
                elif s.kind == "scale":
                    src = _param(s.module.scale, device)
                    sc = _refreshed(tuple(src.shape), torch.float64, src.device, lambda o, src=src: o.copy_(src))
                    pk["scale"][id(s.module)] = sc
                    la = _refreshed((), torch.float64, src.device,
                                    lambda o, sc=sc: torch.sum(sc.abs().log(), dim=0, out=o))
                    pk["ladj_terms"].append((-1.0 if s.inverted else 1.0, la))
                elif s.kind == "coupling":
                    pk["coupling"][i] = self._pack_coupling(i, s.module, device)
                    # (a PLAIN-MLP ConvNet folds its last two Linears on the torch side: the pack cannot be replayed; the general
                    # form -- GatedMLP / LayerNormVector blocks -- packs from the parameters' own storage like a DenseNN)
                    cond_ = s.module.conditioner
                    convnet = convnet or (isinstance(cond_, ConvNet) and (not cond_.is_vector or cond_.is_plain_mlp()))
            pk["ladj_total"] = self._ladj_total(pk)
        # replay needs every source to be the parameter's own storage (no staging copies) and no torch-side folding
        pk["replayable"] = (_copied_params[0] == copies0) and not convnet
        self._pack, self._pack_key = pk, key
        self._plans.clear()
        return pk

    @staticmethod
    def _ladj_total(pk) -> "LogDet":
        """the flow's parameter-only log|det J| as a LogDet: refreshed in place on the device after every parameter
        change, read back to the host only when somebody asks for the Python float"""
        ld = pk.get("ladj_total")
        terms = pk["ladj_terms"]
        if not terms:
            return ld if ld is not None else LogDet(None)
        if "ladj_signs" not in pk:
            pk["ladj_signs"] = torch.tensor([t[0] for t in terms], dtype=torch.float64).to(terms[0][1].device)
        total = (torch.stack([t[1].reshape(()) for t in terms]) * pk["ladj_signs"]).sum()
        if ld is None:
            ld = LogDet(torch.empty((), dtype=torch.float64, device=total.device))
        ld.refresh(total)
        return ld

    def _pk_record(self, pk):
        """context: launches of a lazily built pack item join the pack's tape (refreshed on replay)"""
        return _ext.record(pk["tape"] if pk.get("replayable") else None)

    def _pack_coupling(self, i: int, layer, device) -> dict:
        """Static description of one coupling layer + handles to its raw conditioner parameters; the weight images
        themselves (unfused: ``_unfused_pack``, fused: ``_fused_pack`` / ``_fused_pack_bwd``) are built on first use
        by ``usf_pack_weight_f32`` launches (mask-aware column / row selection, zero padding, bf16x3 planes)."""
        cond = layer.conditioner
        flip = self._flip[i]
        # mask==1 features condition, mask==0 features are transformed (transforms.py:285-290)
        if not flip:      # layer mask == base mask: pass = segment 1, transformed = segment 0
            pass_off, pass_n, pass_idx = self.n0a, self.n1a, self.seg_idx[self.n0a: self.n0a + self.n1a]
            tr_off, tr_n, tr_idx = 0, self.n0, self.seg_idx[: self.n0]
        else:
            pass_off, pass_n, pass_idx = 0, self.n0a, self.seg_idx[: self.n0a]
            tr_off, tr_n, tr_idx = self.n0a, self.n1, self.seg_idx[self.n0a: self.n0a + self.n1]
        act, slope = _activation_of(cond.f)
        has_ctx = isinstance(cond, ConditionalDenseNN)
        if isinstance(cond, ConvNet) and not cond.is_plain_mlp():
            # Linear, [GatedMLP | (f, Linear)] [+ LayerNormVector] x n, Linear (networks.py:287-308)
            first, blocks, final = cond.block_view()
            P = lambda l: (_param(l.weight, device), _param(l.bias, device))     # noqa: E731
            raw = dict(first=P(first), last=P(final), device=device, ctx=None, h=[int(first.out_features)],
                       pass_idx=pass_idx.to(torch.int32), tr_idx=tr_idx.to(torch.int32),
                       blocks=[dict(w_in=int(b["w_in"]), w_out=int(b["w_out"]), eps=(float(b["ln"].eps) if b["ln"] is not None else 0.0),
                                    **{k_: P(b[k_]) for k_ in ("lin", "l1", "l2", "proj", "ln") if b.get(k_) is not None})
                               for b in blocks])
            return dict(pass_off=pass_off, pass_n=pass_n, tr_off=tr_off, tr_n=tr_n, act=act, slope=slope, general=True,
                        hidden=[_round_up(int(w), 4) for w in [first.out_features] + list(cond.c_hidden)], has_ctx=False, raw=raw)
        if isinstance(cond, ConvNet):
            # Linear, [f, Linear] x n, Linear (networks.py:287-308): the last block's Linear and the final Linear
            # have no activation between them -> one output map, folded in fp64
            first, hidden, (W_last, b_last), widths = cond.mlp_view()
            W_last, b_last = W_last.to(device).contiguous(), b_last.to(device).contiguous()
        else:
            first, ctx_l, hidden, last = conditioner_layers(cond)
            W_last, b_last = _param(last.weight, device), _param(last.bias, device)
            widths = cond.hidden_dims
        h = [int(x) for x in widths]
        hp = [_round_up(x, 4) for x in h]
        raw = dict(first=(_param(first.weight, device), _param(first.bias, device)),
                   hidden=[(_param(l.weight, device), _param(l.bias, device)) for l in hidden],
                   last=(W_last, b_last), h=h, device=device,
                   pass_idx=pass_idx.to(torch.int32), tr_idx=tr_idx.to(torch.int32),
                   ctx=(_param(ctx_l.weight, device), _param(ctx_l.bias, device)) if has_ctx else None)
        return dict(pass_off=pass_off, pass_n=pass_n, tr_off=tr_off, tr_n=tr_n, act=act, slope=slope,
                    hidden=hp, has_ctx=has_ctx, raw=raw)

    def _sel(self, idx: torch.Tensor, n_total: int, device) -> torch.Tensor:
        """int32 device selector: idx (feature numbers, -1 = padding) extended with -1 to n_total"""
        t = torch.full((n_total,), -1, dtype=torch.int32)
        t[: idx.numel()] = idx
        return t.to(device)

    def _packed(self, src, out_sel, n_out, in_sel, n_in, planes_sel=None, planes_ld=0, want_w=True, transpose=False):
        """(W [n_out, n_in] fp32 | None, planes [3, n_out, planes_ld] bf16 | None) from a raw parameter; transpose: the
        image of src^T (out_sel picks columns of src, in_sel rows)"""
        dev = src.device
        W = torch.empty(n_out, n_in, dtype=torch.float32, device=dev) if want_w else None
        kw = dict(transpose=True) if transpose else {}
        if W is not None:
            _ext.pack_weight(src, out_sel, n_out, in_sel, n_in, W=W, ldw=n_in, **kw)
        planes = None
        if planes_ld:
            planes = torch.empty(3, n_out, planes_ld, dtype=torch.bfloat16, device=dev)
            _ext.pack_weight(src, out_sel, n_out, in_sel if planes_sel is None else planes_sel,
                             min(n_in, planes_ld) if planes_sel is None else int(planes_sel.numel()), planes=planes, **kw)
        return W, planes

    def _packed_vec(self, src, sel, n) -> torch.Tensor:
        out = torch.empty(n, dtype=torch.float32, device=src.device)
        _ext.pack_weight(src.reshape(1, -1), None, 1, sel, n, W=out, ldw=n, ld_src=src.numel())
        return out

    def _idx_dev(self, layout: str, device) -> torch.Tensor:
        """int32 device copy of the feature index of every column of a layout (-1 = padding column)"""
        cache = self.__dict__.setdefault("_idx_cache", {})
        key = (layout, str(device))
        if key not in cache:
            cache[key] = self._idx(layout).to(device=device, dtype=torch.int32)
        return cache[key]

    def _iarange(self, n_valid: int, n_total: int, device) -> torch.Tensor:
        """int32 [0 .. n_valid-1, -1, -1, ...] of length n_total (row/column selector with zero padding)"""
        cache = self.__dict__.setdefault("_idx_cache", {})
        key = ("arange", n_valid, n_total, str(device))
        if key not in cache:
            t = torch.full((n_total,), -1, dtype=torch.int32)
            t[:n_valid] = torch.arange(n_valid, dtype=torch.int32)
            cache[key] = t.to(device)
        return cache[key]

    def _wants_planes(self, n_out: int, K: int) -> bool:
        return self.gemm_mode in ("bf16x3", "f16x2") and K % 8 == 0 and n_out > 64

    def _mat(self, pk, blk, which: str, out_layout: str, in_layout: str, transpose: bool = False) -> torch.Tensor:
        """permuted / padded fp32 image [n_out, n_in] of an affine block's M or M^-1 (+ its bf16x3 planes), one launch;
        transpose: the image [n_in, n_out] of its transpose -- the data-gradient operand of the training backward"""
        key = (id(blk), which, out_layout, in_layout) + (("T",) if transpose else ())
        if key not in pk["mats"]:
            src = pk["affine"][id(blk)][which]
            dev = src.device
            rows, cols = self._idx_dev(out_layout, dev), self._idx_dev(in_layout, dev)
            kw = {}
            if transpose:
                rows, cols, kw = cols, rows, dict(transpose=True)
            n_r, n_c = int(rows.numel()), int(cols.numel())
            W = torch.empty(n_r, n_c, dtype=torch.float32, device=dev)
            planes = None
            if self._wants_planes(n_r, n_c):
                planes = torch.empty(3, n_r, _round_up(n_c, 32), dtype=torch.bfloat16, device=dev)
            with self._pk_record(pk):
                _ext.pack_weight(src, rows, n_r, cols, n_c, W=W, ldw=n_c, planes=planes, **kw)
            pk["mats"][key] = W
            if planes is not None:
                pk["mats"][("planes", W.data_ptr())] = planes
        return pk["mats"][key]

    def _split_kw(self, pk, W: torch.Tensor, K: int) -> dict:
        """descriptor fields that hand the bf16x3 planes of W to usf_linear_f32 (empty in f32 mode)"""
        if not self._wants_planes(W.shape[0], K):
            return {}
        planes = self._split_planes(pk, W)
        return dict(W_split=planes.data_ptr(), ldw_split=planes.shape[2],
                    split_plane_stride=planes.shape[1] * planes.shape[2])

    @staticmethod
    def _split_planes(pk, W: torch.Tensor) -> torch.Tensor:
        """[3, N, ceil32(K)] bf16 planes with W1 + W2 + W3 == W (round-to-nearest residual split)"""
        key = ("planes", W.data_ptr())
        if key not in pk["mats"]:
            N, K = W.shape
            planes = torch.empty(3, N, _round_up(K, 32), dtype=torch.bfloat16, device=W.device)
            with _ext.record(pk["tape"] if pk.get("replayable") else None):
                _ext.flush_jobs()              # W itself may be the output of a queued job
                _ext.pack_weight(W, None, N, None, K, planes=planes)
            pk["mats"][key] = planes
        return pk["mats"][key]

    def _vec(self, pk, name, v64, layout: str, pad: float) -> torch.Tensor:
        key = (name, layout, pad)
        if key not in pk["vecs"]:
            with self._pk_record(pk):
                if pad == 0.0:
                    idx = self._idx_dev(layout, v64.device)
                    out = torch.empty(idx.numel(), dtype=torch.float32, device=v64.device)
                    _ext.pack_weight(v64, None, 1, idx, int(idx.numel()), W=out, ldw=int(idx.numel()))
                    pk["vecs"][key] = out
                else:
                    n = int(self._idx(layout).numel())
                    pk["vecs"][key] = _refreshed((n,), torch.float32, v64.device,
                                                 lambda o: o.copy_(self._perm_vec(v64, self._idx_dev(layout, v64.device), pad)))
        return pk["vecs"][key]

    # ---- workspace ----------------------------------------------------------------------------
    def _workspace(self, B: int, device) -> Dict[str, torch.Tensor]:
        key = (B, str(device))
        ws = self._ws.get(key)
        if ws is None:
            if len(self._ws) > 4:
                self._ws.clear()
                self._plans.clear()
            z = lambda *shape: torch.zeros(*shape, dtype=torch.float32, device=device)
            ws = dict(zA=z(B, self.LD), zB=z(B, self.LD), nat=z(B, self.LDn), H1=z(B, self.hmax),
                      H2=z(B, self.hmax), P=z(B, self.hmax), ctx4=z(B, _round_up(self.ctx_dim, 4)),
                      sum=torch.zeros(2, dtype=torch.float64, device=device))
            if self.ctx_dim == 1:
                ws["ctx"] = z(B)
            # (ctx4 [B, Cp]: the context rows, 16-byte aligned, columns [C, Cp) zero -- the operand of the unfused plan's context
            # GEMM and, for C > 1, of the fused kernels' vector form; ctx [B]: the scalar form's column, C == 1 only)
            self._ws[key] = ws
        return ws

    def _nat2(self, ws, B: int, device) -> torch.Tensor:
        """ws["nat2"] [B, LDn], made on first use: where a plan of either builder leaves its fp32 result for the workspace
        (final = 'nat'; "nat" itself may be the staging copy of the input)"""
        if "nat2" not in ws:
            ws["nat2"] = torch.zeros(B, self.LDn, dtype=torch.float32, device=device)
        return ws["nat2"]

    # ---- plan construction --------------------------------------------------------------------
    def _step(self, i: int) -> _Step:
        return self.steps[i] if i < len(self.steps) else self._virtual[i - len(self.steps)]

    def _merge_on(self, direction: str, device=None) -> bool:
        """are runs of consecutive affine maps composed in this direction's inference plans right now?"""
        if self.merge_affine != "auto":
            return bool(self.merge_affine)
        pk = self._pack
        return bool(pk is not None and pk.get("auto_merge", {}).get(direction, False))

    def resolve_merge(self, direction: str, x: torch.Tensor, runner=None) -> bool:
        """merge_affine == "auto": decide, once per pack and direction, whether this flow's runs of consecutive affine
        maps may be composed.  The probe is end to end -- up to 64 rows of the caller's own batch through the plan with
        composed runs and through the layer-by-layer plan: the composite itself is as accurate as its parts (both are
        rounded once from fp64 factors), what differs between flows is how far ANY change of rounding pattern is
        amplified downstream.  Where the two results agree (1e-5 of the largest output element-wise, 1e-6 in the rows'
        L1 norms -- half resp. a tenth of what the parity bars allow; measured: the reference's default-initialised
        golden flows 4e-6 .. 1.4e-5 in the L1 measure, conditioned flows up to the 65-layer cfg2 model 1e-7 .. 4e-7)
        the flow is well conditioned
        and the composed plan (half the D x D GEMMs of a conjugated flow) is indistinguishable from the reference's
        arithmetic at the 1e-5 parity bar; where they do not (default-initialised, exploding flows: the reference's
        own fp32 run is 2 - 7e-6 from its fp64 run there) the layers keep their own launches.  Costs two 64-row passes
        and one scalar read-back at the first inference call after a (re)pack; re-probed every 256 in-place refreshes.
        runner(plan, x, out): how a plan is executed (tests interpret the op list on the CPU)."""
        if self.merge_affine != "auto":
            return bool(self.merge_affine)
        pk = self.pack(x.device)
        state = pk.setdefault("auto_merge", {})
        if direction in state:
            return state[direction]
        if x.is_cuda and torch.cuda.is_current_stream_capturing():
            return False          # (the probe reads a scalar back: never inside a caller's stream capture -- this call keeps
            #                        the layer-by-layer plan, the next call outside a capture decides)
        has_run = any(a.startswith("affine") and b_.startswith("affine")
                      for (a, _), (b_, _) in zip(self._primitive_ops(direction)[:-1], self._primitive_ops(direction)[1:]))
        if not has_run or x.shape[0] == 0:
            state[direction] = False
            return False
        run = runner if runner is not None else (lambda plan, xs, out: self._run(plan, xs, out, None))
        n = min(64, x.shape[0])
        xs = x[:n].contiguous()
        outs = []
        with torch.no_grad():
            for mode in (False, True):
                state[direction] = mode
                out = torch.empty(n, self.D, dtype=torch.float32, device=x.device)
                run(self._plan(direction, n, x.device, False, "user"), xs, out)
                outs.append(out.double())
            # two measures: the largest element-wise deviation against the largest output (the parity tests allow 2e-5 of
            # it), and the deviation of the rows' L1 norms -- what a Laplace / radial base density sums, i.e. the log_prob's
            # sensitivity (bar: 1e-5 relative)
            d = ((outs[1] - outs[0]).abs().max() / outs[0].abs().max().clamp_min(1e-30)).item()
            l1 = outs[0].abs().sum(-1)
            d1 = ((outs[1].abs().sum(-1) - l1).abs() / l1.clamp_min(1e-30)).max().item()
        ok = bool(d <= 1e-5 and d1 <= 1e-6)               # (NaN / inf compare False)
        self.merge_guard_log.append((ok, d, d1))
        state[direction] = ok
        return ok

    def _primitive_ops(self, direction: str, merge: bool = False):
        """[(prim, step_index)] with prim in scale_mul/scale_div/affine_fwd/affine_bwd/coupling_fwd/coupling_bwd;
        merge: runs of consecutive affine steps become one ``affine_fwd`` on a ``_MergedAffine`` (``_step(index)``) when
        merging is on for this direction (``_merge_on``: merge_affine True, or "auto" and the probe accepted)"""
        seq = list(enumerate(self.steps))
        if direction == "backward":
            seq = seq[::-1]
        prims = []
        for i, s in seq:
            fwd = (direction == "forward") != s.inverted
            if s.kind == "scale":
                prims.append(("scale_mul" if fwd else "scale_div", i))
            elif s.kind == "affine":
                prims.append(("affine_fwd" if fwd else "affine_bwd", i))
            else:
                prims.append(("coupling_fwd" if fwd else "coupling_bwd", i))
        if not (merge and self._merge_on(direction)):
            return prims
        out, k = [], 0
        while k < len(prims):
            j = k
            while j < len(prims) and prims[j][0] in ("affine_fwd", "affine_bwd"):
                j += 1
            if j - k >= 2:
                parts = [(p_, self.steps[i_].module) for p_, i_ in prims[k:j]]
                key = tuple((p_, id(b_)) for p_, b_ in parts)
                if key not in self._virtual_ix:
                    self._virtual.append(_Step("affine", _MergedAffine(parts), False))
                    self._virtual_ix[key] = len(self.steps) + len(self._virtual) - 1
                out.append(("affine_fwd", self._virtual_ix[key]))
                k = j
            else:
                out.append(prims[k])
                k += 1
        return out

    def _affine_entry(self, pk, blk) -> dict:
        """pk["affine"] entry of a block; a merged run is composed here on first use (fp64, launches on the pack's tape:
        refreshed in place with the parameters)"""
        if id(blk) in pk["affine"] or not isinstance(blk, _MergedAffine):
            return pk["affine"][id(blk)]
        with self._pk_record(pk):
            _ext.flush_jobs()
            W = c = None
            for prim, b_ in blk.parts:
                a = pk["affine"][id(b_)]
                if prim == "affine_fwd":
                    Wk, ck = a["M"], a["b"]
                else:
                    Wk, ck = a["Minv"], folded_bias(a)
                if W is None:
                    W, c = Wk, ck
                else:
                    W = _ext.matmul_f64(Wk.contiguous(), W.contiguous())
                    t = torch.empty(ck.shape, dtype=torch.float64, device=ck.device)
                    _ext.matvec_f64(Wk.contiguous(), c.contiguous(), alpha=1.0, out64=t)
                    c = _refreshed(tuple(ck.shape), torch.float64, ck.device,
                                   lambda o, t=t, ck=ck: torch.add(t, ck, out=o))
            pk["affine"][id(blk)] = dict(M=W, b=c)
        return pk["affine"][id(blk)]

    def _build_plan(self, direction: str, B: int, device, has_ctx: bool, final: str, train: bool = False) -> dict:
        # every weight image the plan needs is queued while the op list is laid out and packed by ONE batched launch
        # per size class at the end (nothing reads them before the plan runs); the launch joins the pack's tape
        pk = self.pack(device)
        with self._pk_record(pk), _ext.batch_jobs(device):
            if self._planes_ok(direction, B, has_ctx, train):
                return self._build_plan_planes(direction, B, device, final, train, has_ctx)
            return self._build_plan_body(direction, B, device, has_ctx, final, train)

    # ---- execution ----------------------------------------------------------------------------
    def _plan(self, direction, B, device, has_ctx, final, train: bool = False):
        pk = self.pack(device)   # may invalidate plans
        key = (direction, B, str(device), has_ctx, final, self.use_fused_coupling, self.gemm_mode, self.fused_min_rows,
               config.tiny_coupling, config.get_lib("coupling_tiny", 1), train, self.use_planes, self.planes_min_rows, self._planes_fmt(), self.planes_min_rows_bf16x3,
               (not train) and self._merge_on(direction), train and self.use_train_planes, train and self.train_planes_min_rows,
               has_ctx and (self.train_ctx_planes_min_rows if train else self.ctx_planes_min_rows), has_ctx and self.ctx_dim,
               (not train) and self.planes_side_f32 and B >= self.planes_side_min_rows)
        plan = self._plans.get(key)
        if plan is None:
            plan = self._build_plan(direction, B, device, has_ctx, final, train)
            self._plans[key] = plan
        return plan

    def _run_guarded(self, direction, x, out, context, final):
        """plan + run; a planes pass in fp16x2 format whose range guard fired (a NaN or |value| >= 65000 somewhere in
        the flow: fp16 planes cannot carry it) is void and is redone with bf16x3 planes.  The check reads one int32
        back from the device, i.e. it waits for the pass: only plans of >= planes_min_rows rows (milliseconds) do it."""
        B = x.shape[0]
        if self.merge_affine == "auto" and context is None:
            self.resolve_merge(direction, x)
        plan = self._plan(direction, B, x.device, context is not None, final)
        self._run(plan, x, out, context)
        if plan.get("planes_fmt") == _ext.PLANES_F16X2 and int(plan["ws"]["pflag"].item()) != 0:
            plan["ws"]["pflag"].zero_()
            self.f16_fallbacks += 1
            self._f16_overflow = True
            try:
                if final.startswith("base") and not self._planes_ok(direction, B, context is not None, False):
                    # the bf16x3 redo is no planes plan (a context on a conditioner bf16x3 does not run fused): nothing reduces
                    # the base density in an epilogue there -- latent_base_sums hands the batch back to latent + the density pass
                    return None
                plan = self._plan(direction, B, x.device, context is not None, final)
                self._run(plan, x, out, context)
            finally:
                self._f16_overflow = False
        return plan

    def _run(self, plan, x: torch.Tensor, out: Optional[torch.Tensor], context):
        """every pass over a workspace -- training forward or no_grad evaluation, they share the (B, device) buffers --
        bumps its generation counter: activations a training forward left there are stale afterwards, and the
        training backward re-runs its forward when it finds the counter moved (training.py)"""
        ws = plan["ws"]
        ws["_gen"] = ws.get("_gen", 0) + 1
        self._execute(plan, x, out, context)

    def _execute(self, plan, x: torch.Tensor, out: Optional[torch.Tensor], context):
        """run the plan's launches on torch's current stream; small batches replay them as ONE hipGraph"""
        if (self.use_graphs and x.shape[0] <= self.graph_max_rows and self.op_timing is None
                and not torch.cuda.is_current_stream_capturing()):
            return self._execute_graph(plan, x, out, context)
        return self._execute_plain(plan, x, out, context)

    def _execute_graph(self, plan, x, out, context):
        """Launch-bound regime (B <= graph_max_rows: ~130 launches of a few microseconds each): the launch list is
        captured once into a hipGraph (torch.cuda.CUDAGraph over the C-ABI launches -- they go to the capturing
        stream) and replayed; the caller's tensors are staged through fixed buffers so the captured pointers stay
        valid.  An in-place pack refresh (new parameter values, same addresses) keeps the graph valid."""
        ws = plan["ws"]
        B = x.shape[0]
        if "x_static" not in ws:
            ws["x_static"] = torch.empty(B, self.D, dtype=torch.float32, device=x.device)
        xs = ws["x_static"]
        xs.copy_(x)
        os_ = None
        if out is not None:
            if "out_static" not in ws:
                ws["out_static"] = torch.empty(B, self.D, dtype=torch.float32, device=x.device)
            os_ = ws["out_static"]
        if context is not None:
            self._fill_context(plan, context, B)
        g = plan.get("graph")
        if g is None:
            if plan.get("graph_warm", 0) < 1:
                # first call: plain launches (builds every lazily packed weight image before anything is captured)
                plan["graph_warm"] = 1
                self._execute_plain(plan, xs, os_, None)
            else:
                torch.cuda.synchronize(x.device)
                g = torch.cuda.CUDAGraph()
                with _ext.capture_without_gc(), torch.cuda.graph(g):
                    self._execute_plain(plan, xs, os_, None)
                plan["graph"] = g
                g.replay()
        else:
            g.replay()
            self.launch_count += 1
        if out is not None:
            out.copy_(os_)

    def _fill_context(self, plan, context, B: int):
        """the context columns of the workspace: one value per row ([B] / [B, 1]), or ONE value spread over the rows (the plans'
        launches read them with stride 1; stride 0 of usf_coupling_planes_ctx is for direct callers of the entry point).
        context_dim C > 1: rows of C values ([B, C]), or ONE row ([1, C] / [C]) spread over the rows, of any floating dtype, into
        columns [0, C) of ctx4 [B, Cp]; the padding columns keep their zeros."""
        ws = plan["ws"]
        Cd = self.ctx_dim
        if Cd > 1:
            if tuple(context.shape) not in ((B, Cd), (1, Cd), (Cd,)):        # the shapes the reference's layers[1] broadcasts
                raise ValueError(f"context of shape {tuple(context.shape)}: a context_dim {Cd} flow takes [{B}, {Cd}], [1, {Cd}] "
                                 f"or [{Cd}] for {B} rows")
            ws["ctx4"][:, :Cd].copy_(context.reshape(-1, Cd).expand(B, Cd))       # (copy_ converts any floating dtype)
            return
        c = context.reshape(-1).to(torch.float32)
        if c.numel() == 1 and B > 1:
            c = c.expand(B)
        ws["ctx4"][:, 0].copy_(c)
        ws["ctx"].copy_(c)

    def _execute_plain(self, plan, x: torch.Tensor, out: Optional[torch.Tensor], context):
        ws = plan["ws"]
        B = x.shape[0]
        dev = x.device
        if context is not None:
            self._fill_context(plan, context, B)
        arr = plan["arr"]
        for idx, member, field in plan["patch_in"]:
            setattr(getattr(arr[idx].u, member), field, x.data_ptr())
        for idx, member, field in plan["patch_out"]:
            setattr(getattr(arr[idx].u, member), field, out.data_ptr())
        lib = _ext.load()
        stream = _ext.current_stream(dev)
        pos = 0

        def run_until(end):
            nonlocal pos
            if end > pos and self.op_timing is not None:
                # instrumented mode: one launch per call, bracketed by HIP events on the launch stream
                j = pos
                while j < end:
                    op = arr[j]
                    n_run = 2 if _ext.is_ctx_prefix(op) else 1       # (a context prefix and its coupling op are ONE launch)
                    side = _ext.is_side_prefix(op)                   # (so are a side-buffer prefix and its planes op, under that op's tag)
                    if side:
                        n_run, op = 2, arr[j + 1]
                    if n_run == 2 and not side and arr[j + 1].kind == _ext.OP_COUPLING:
                        c_ = arr[j + 1].u.coupling
                        tag = ("coupling_vctx", c_.M, c_.n_trans, c_.n_pass)
                    elif n_run == 2 and not side:
                        c_ = arr[j + 1].u.coupling_planes
                        tag = ("coupling_planes_ctx", c_.M, 32 * c_.nk_t, 32 * c_.nk_p)
                    elif op.kind == _ext.OP_LINEAR:
                        kind = "linear_bf16x3" if op.u.linear.W_split else "linear"
                        tag = (kind, op.u.linear.M, op.u.linear.N, op.u.linear.K)
                    elif op.kind == _ext.OP_GEMM_PLANES:
                        g_ = op.u.gemm_planes
                        tag = ("gemm_planes", g_.M, g_.N if g_.C_f32 else 32 * g_.c_kbn, 32 * g_.nk)
                    elif op.kind == _ext.OP_PACK_PLANES:
                        tag = ("pack_planes", op.u.pack_planes.M, 32 * op.u.pack_planes.nkb, 0)
                    elif op.kind == _ext.OP_COUPLING_PLANES:
                        c_ = op.u.coupling_planes
                        tag = ("coupling_planes", c_.M, 32 * c_.nk_t, 32 * c_.nk_p)
                    else:
                        tag = ("coupling", op.u.coupling.M, op.u.coupling.n_trans, op.u.coupling.n_pass)
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    sub = C.cast(C.byref(arr, j * C.sizeof(_ext.Op)), C.POINTER(_ext.Op))
                    _ext.check(lib.usf_run_ops(sub, n_run, stream), "usf_run_ops")
                    e1.record()
                    self.op_timing.append((tag, e0, e1))
                    j += n_run
                self.launch_count += 1
                pos = end
            elif end > pos:
                sub = C.cast(C.byref(arr, pos * C.sizeof(_ext.Op)), C.POINTER(_ext.Op))
                _ext.check(lib.usf_run_ops(sub, end - pos, stream), "usf_run_ops")
                self.launch_count += 1
                pos = end

        for g in plan["side"]:           # already in op order (stable)
            run_until(g[1])
            if g[0] == "scale":
                _, _, buf, ld, sc, divide, ncols = g
                _ext.scale(ws[buf], ld, ws[buf], ld, B, ncols, sc, divide)
                self.launch_count += 1
            else:
                _, _, src, dst_name, dst_layout = g
                src_t = x if src[0] == "user_in" else ws[src[0]]
                idx = self._gather_index(src[1], dst_layout, dev)
                dst_t = ws[dst_name]
                _ext.gather_cols(src_t, src[2], dst_t, dst_t.shape[1], B, dst_t.shape[1], idx)
                self.launch_count += 1
        run_until(plan["n"])
        fg = plan["final_gather"]
        if fg is not None:
            src, dst_name = fg
            src_t = ws[src[0]]
            if dst_name == "user_out":
                _ext.gather_cols(src_t, src[2], out, self.D, B, self.D, self._gather_index(src[1], "user", dev))
            else:
                _ext.gather_cols(src_t, src[2], ws[dst_name], self.LDn, B, self.LDn,
                                 self._gather_index(src[1], "nat", dev))
            self.launch_count += 1

    def _gather_index(self, src_layout: str, dst_layout: str, device) -> torch.Tensor:
        """int32 index: dst column j <- src column idx[j] (or -1 -> 0)."""
        key = ("gidx", src_layout, dst_layout, str(device))
        cache = self.__dict__.setdefault("_gidx", {})
        if key not in cache:
            src_idx = self._idx(src_layout)
            pos = {int(f): c for c, f in enumerate(src_idx.tolist()) if f >= 0}   # feature -> src column
            if dst_layout == "user":
                feats = list(range(self.D))
            else:
                feats = self._idx(dst_layout).tolist()
            cache[key] = torch.tensor([pos[f] if f >= 0 else -1 for f in feats], dtype=torch.int32, device=device)
        return cache[key]

    # ---- public API ---------------------------------------------------------------------------
    def _check_input(self, x: torch.Tensor) -> torch.Tensor:
        if not x.is_cuda:
            raise RuntimeError("FlowEngine runs on ROCm devices only")
        if x.dim() != 2 or x.shape[1] != self.D:
            raise ValueError(f"expected input of shape [B, {self.D}], got {tuple(x.shape)}")
        if x.dtype != torch.float32:
            x = x.float()
        if not x.is_contiguous() or (x.data_ptr() % 16) != 0:
            x = x.contiguous().clone() if (x.data_ptr() % 16) != 0 else x.contiguous()
        return x

    def transform(self, x: torch.Tensor, direction: str, context: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Flow._forward / Flow.backward on the device: natural layout in, natural layout out."""
        x = self._check_input(x)
        B = x.shape[0]
        out = torch.empty(B, self.D, dtype=torch.float32, device=x.device)
        if B == 0:
            return out
        self._run_guarded(direction, x, out, context, "user")
        return out

    def latent(self, x: torch.Tensor, context=None) -> Tuple[torch.Tensor, int, "LogDet"]:
        """backward pass into the workspace: (z buffer [B, ldn], ldn, the flow's LogDet)."""
        x = self._check_input(x)
        plan = self._run_guarded("backward", x, None, context, "nat")
        buf = plan["ws"][plan["out_buf"][0]]
        return buf, plan["out_buf"][2], plan["pk"]["ladj_total"]

    def latent_base_sums(self, x: torch.Tensor, base: int, loc: torch.Tensor, scale: torch.Tensor, context=None):
        """backward pass with the Laplace / Normal base density reduced by the last GEMM's epilogue (planes plans, D <= 1024):
        (partial sums [B, 8], how many of the 8 are used, the flow's LogDet) -- ``usf_base_logprob_f32(USF_BASE_ROWSUM)`` finishes
        the rows; None when this batch does not take a planes plan (the caller runs ``latent`` + the density pass)."""
        from .config import config
        x = self._check_input(x)
        B = x.shape[0]
        has_ctx = context is not None
        if not (config.base_in_epilogue and self.D <= 1024 and self._planes_ok("backward", B, has_ctx, False)):
            return None
        if self.merge_affine == "auto" and not has_ctx:
            self.resolve_merge("backward", x)
        final = f"base{int(base)}"
        plan = self._plan("backward", B, x.device, has_ctx, final)
        if plan.get("n_part", 0) < 1:
            return None
        ws = plan["ws"]
        _ext.base_tables(base, loc, scale, self.D, ws["btab"], ws["btab"].numel() // 3)
        plan = self._run_guarded("backward", x, None, context, final)
        if plan is None:
            return None
        return plan["ws"]["bpart"], plan["n_part"], plan["pk"]["ladj_total"]

    def ladj_total(self, device) -> float:
        return float(self.pack(device)["ladj_total"])
