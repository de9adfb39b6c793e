"""The planes pipeline's plans: between the dense layers of a flat flow the activations travel as bf16x3
(or fp16x2) planes in a blocked format -- the op lists of ``log_prob`` / ``backward`` / ``_forward`` at large batches and of the
training step on planes (``usf_pack_planes_f32``, ``usf_gemm_planes_bf16x3``, ``usf_coupling_planes``), and the weight / vector images
they read.  A mixin of ``usflows_amd.engine.FlowEngine`` (split out of engine.py in round 5)."""
from __future__ import annotations

from typing import List

import torch

from . import _ext
from ._plan_util import EngineUnsupported, _image_triple, _refreshed, _round_up, affine_span, arange_padded, folded_bias
from .networks import ConditionalDenseNN, ConvNet, DenseNN


class PlanesPlanMixin:
    """see the module docstring"""

    # ---- planes pipeline (usf_planes.hip) ---------------------------------------------------------
    @staticmethod
    def _slot_feature(s_: int) -> int:
        """feature offset (0..31) held by slot s of a 32-feature block of a planes buffer (include/usflows_hip.h)"""
        return 16 * ((s_ & 7) >> 2) + 4 * (s_ >> 3) + (s_ & 3)

    def _phys(self, logical: torch.Tensor) -> torch.Tensor:
        """reorder a per-logical-position selector (length a multiple of 32) into physical slot order"""
        n = int(logical.numel())
        perm = torch.tensor([32 * (c // 32) + self._slot_feature(c % 32) for c in range(n)], dtype=torch.long)
        return logical[perm]

    def _planes_fmt(self) -> int:
        """activation / weight plane format of the planes pipeline: fp16x2 in "f16x2" mode (three MFMAs per product,
        22 significant bits per operand) unless a pass just overflowed fp16's range, bf16x3 otherwise"""
        return _ext.PLANES_F16X2 if (self.gemm_mode == "f16x2" and not self._f16_overflow) else _ext.PLANES_BF16X3

    def _planes_ok(self, direction: str, B: int, has_ctx: bool, train: bool) -> bool:
        if has_ctx and self.ctx_dim > 1:
            return False       # a vector context never takes the planes plans (usf_coupling_planes_ctx is rank-1), also in training
        if self.use_planes is None:
            use = self.gemm_mode == "f16x2" or B >= self.planes_min_rows_bf16x3 or self._has_wide_conditioner()
            if has_ctx:        # (off until measured: engine.py, ctx_planes_min_rows)
                use = use and self.ctx_planes_min_rows is not None and B >= self.ctx_planes_min_rows
        else:
            use = bool(self.use_planes)
        if train:
            # the training step on the planes pipeline (round 5; training_planes.py `backward_body`): log_prob plans in the bf16x3
            # format whose couplings all run as ONE fused launch (conditioners of <= 2 hidden layers up to 256 wide), from
            # train_planes_min_rows rows; every planes buffer below 2 GiB (usf_wgrad_blocked_f32's offsets)
            use = (self.use_train_planes and direction == "backward" and self.gemm_mode == "bf16x3" and self.use_fused_coupling
                   and B >= max(self.train_planes_min_rows, self.fused_min_rows)
                   and (-(-B // 16)) * (self.LDp // 32) * 3072 < 2 ** 31 and self._train_planes_conditioners_ok()
                   and (not has_ctx or (self.train_ctx_planes_min_rows is not None and B >= self.train_ctx_planes_min_rows)))
        if (not use or self._general_cond or self.gemm_mode not in ("bf16x3", "f16x2")
                or B < self.planes_min_rows or (-(-B // 16)) * (self.LDp // 32) * 3072 >= 2 ** 32):
            return False
        if has_ctx and not self._planes_ctx_ok(B):
            return False
        # (the structure check does not depend on which runs are merged: a merged run is an affine step like its parts)
        prims = self._primitive_ops(direction, merge=False)
        kinds = [p_[0] for p_ in prims]
        for k_, kind in enumerate(kinds):
            if kind == "scale_div" and not (k_ == 0 and len(kinds) > 1 and kinds[1] in ("affine_bwd", "affine_fwd")):
                return False
            if kind == "scale_mul" and not (k_ == len(kinds) - 1 and k_ > 0 and kinds[k_ - 1] == "affine_fwd"):
                return False
        body = [k_ for k_ in kinds if not k_.startswith("scale")]
        # the last layer must be an affine (it writes the fp32 result) and the chain needs at least two GEMM-sized ops
        return len(body) >= 2 and body[-1].startswith("affine")

    def _planes_coupling_fused(self, h, B: int, fmt: int) -> bool:
        """a coupling whose conditioner has the hidden widths h runs as ONE usf_coupling_planes launch in a planes plan of B rows"""
        return (self.use_fused_coupling and B >= self.fused_min_rows and len(h) <= 3 and max(h) <= 256
                and not (fmt == _ext.PLANES_BF16X3 and len(h) == 3))

    def _planes_ctx_ok(self, B: int) -> bool:
        """a context rides the planes pipeline only inside the fused coupling launch (usf_coupling_planes_ctx: a start value of
        the first layer's accumulators): every conditioner WITH a context layer must run fused.  Otherwise -- bf16x3 with three
        hidden layers, conditioners wider than 256, use_fused_coupling off -- the flow keeps the fp32-activation plan."""
        fmt = self._planes_fmt()
        for s_ in self.steps:
            if s_.kind == "coupling" and isinstance(s_.module.conditioner, ConditionalDenseNN):
                if not self._planes_coupling_fused([int(w) for w in s_.module.conditioner.hidden_dims], B, fmt):
                    return False
        return True

    def _train_planes_conditioners_ok(self) -> bool:
        # (the weight-gradient kernel carries the bias sums along only for operands of >= 64 columns -- usf_wgrad_planes_colsum_ok --:
        # flows whose halves are narrower keep the fp32-row training path, which is made for them)
        if min(self.n0a, self.n1a) < 64:
            return False
        for s_ in self.steps:
            if s_.kind == "coupling":
                cond = s_.module.conditioner
                if not isinstance(cond, (ConditionalDenseNN, DenseNN)):
                    return False
                widths = [int(w) for w in cond.hidden_dims]
                if len(widths) > 2 or max(widths) > 256:
                    return False
        return True

    def _has_wide_conditioner(self) -> bool:
        """a conditioner wider than 256 or deeper than 3 hidden layers: no fused coupling kernel serves it"""
        for s_ in self.steps:
            if s_.kind == "coupling":
                cond = s_.module.conditioner
                widths = cond.c_hidden if isinstance(cond, ConvNet) else cond.hidden_dims
                if len(widths) > 3 or max(int(w) for w in widths) > 256:
                    return True
        return False

    def _planes_image(self, pk, key, src, out_sel: torch.Tensor, in_sel: torch.Tensor, fmt: int = 0, transpose: bool = False):
        """cached weight planes of src[out_sel][:, in_sel] (-1: zero; transpose: of src[in_sel][:, out_sel]^T), one queued
        launch: [3, rows, cols] bf16 (bf16x3) or [2, rows, cols] fp16 (fp16x2)"""
        mats = pk["mats"]
        key = key + (fmt,) + (("T",) if transpose else ())
        if key not in mats:
            dev = src.device
            n_out, n_in = int(out_sel.numel()), int(in_sel.numel())
            if fmt == _ext.PLANES_F16X2:
                P = torch.empty(2, n_out, n_in, dtype=torch.float16, device=dev)
            else:
                P = torch.empty(3, n_out, n_in, dtype=torch.bfloat16, device=dev)
            _ext.pack_weight(src, out_sel.to(device=dev, dtype=torch.int32), n_out,
                             in_sel.to(device=dev, dtype=torch.int32), n_in, planes=P, transpose=transpose)
            mats[key] = P
        return mats[key]

    def _planes_vec(self, pk, key, src, sel: torch.Tensor, pad: float = 0.0) -> torch.Tensor:
        """cached fp32 vector src[sel] (-1: pad) of length len(sel)"""
        vecs = pk["vecs"]
        if key not in vecs:
            dev = src.device
            n = int(sel.numel())
            if pad == 0.0:
                out = torch.empty(n, dtype=torch.float32, device=dev)
                _ext.pack_weight(src.reshape(1, -1), None, 1, sel.to(device=dev, dtype=torch.int32), n, W=out, ldw=n,
                                 ld_src=src.numel())
                vecs[key] = out
            else:
                sel_dev = sel.to(dev)                    # (once: a host index in the refresh would synchronise every step)
                vecs[key] = _refreshed((n,), torch.float32, dev,
                                       lambda o, src=src, sel=sel_dev: o.copy_(self._perm_vec(src.double(), sel, pad)))
        return vecs[key]

    # ---- a coupling on planes: its block ranges, its weight images (both directions), its descriptor --------------------
    def _coupling_geometry(self, cp) -> dict:
        """where a coupling layer lives in a planes buffer of the segment layout: the block ranges of its conditioning (p) and
        transformed (t) features, their valid widths relative to the range's first block, and the feature number of every
        position of the buffer that belongs to either set (-1 elsewhere).  Goes into the coupling's ``meta`` entry as it is."""
        segp = self.segp_idx
        lo_p, hi_p = cp["pass_off"], cp["pass_off"] + int((cp["raw"]["pass_idx"] >= 0).sum())
        lo_t, hi_t = cp["tr_off"], cp["tr_off"] + cp["tr_n"]
        kb_p0, kb_t0 = lo_p // 32, lo_t // 32
        pos = torch.arange(self.LDp)
        none = torch.full_like(segp, -1)
        return dict(kb_p0=kb_p0, nk_p=-(-hi_p // 32) - kb_p0, kb_t0=kb_t0, nk_t=-(-hi_t // 32) - kb_t0,
                    n_p=hi_p - 32 * kb_p0, n_t=hi_t - 32 * kb_t0,
                    feat_p=torch.where((pos >= lo_p) & (pos < hi_p), segp, none),
                    feat_t=torch.where((pos >= lo_t) & (pos < hi_t), segp, none))

    def _coupling_planes_images(self, pk, i: int, geo: dict, fmt: int, backward: bool = False) -> dict:
        """the weight images of usf_coupling_planes for coupling step i (hidden widths padded to 256, K axes in slot order).
        Forward: the conditioner's layers in order with their bias vectors.  backward (USF_ACT_GATE): the same chain run from
        the transformed blocks to the conditioning blocks -- W_in = W_last^T, the hidden matrices reversed and transposed,
        W_out = W_first^T -- with one shared zero vector for every bias."""
        raw = pk["coupling"][i]["raw"]
        h = list(raw["h"])
        layers = [raw["first"]] + list(raw["hidden"]) + [raw["last"]]
        # the index set at both ends of every layer: layer j maps ends[j] -> ends[j + 1]
        ends = ([geo["feat_p"][32 * geo["kb_p0"]: 32 * (geo["kb_p0"] + geo["nk_p"])]] + [arange_padded(w, 256) for w in h]
                + [geo["feat_t"][32 * geo["kb_t0"]: 32 * (geo["kb_t0"] + geo["nk_t"])]])
        n = len(layers)
        mats, vecs = [], []
        if backward:
            zeros = torch.zeros(max(256, int(ends[0].numel())), dtype=torch.float32, device=raw["device"])
        for at, j in enumerate(reversed(range(n)) if backward else range(n)):
            role = "in" if at == 0 else ("out" if at == n - 1 else "hid")         # (the cache keys name the role in the launch)
            jkey = (i, j) if role == "hid" else (i,)
            out_sel, in_sel = (ends[j], ends[j + 1]) if backward else (ends[j + 1], ends[j])
            mats.append(self._planes_image(pk, (f"pl_c{role}_t" if backward else f"pl_c{role}",) + jkey, layers[j][0], out_sel,
                                           self._phys(in_sel), fmt, transpose=backward))
            vecs.append(zeros if backward else self._planes_vec(pk, (f"pl_c{role}b",) + jkey, layers[j][1], out_sel))
        f = dict(W_in=mats[0], hid=mats[1:-1], W_out=mats[-1], b_in=vecs[0], b_hid=vecs[1:-1], b_out=vecs[-1])
        if backward:
            f["zeros"] = zeros
        return f

    # ---- training on the planes pipeline: the backward launches' weight images (training_planes.py `backward_body`) ----
    def planes_dgrad_image(self, pk, m) -> torch.Tensor:
        """weight planes of an affine layer's data gradient g_in = g_out W as a usf_gemm_planes_bf16x3 operand: rows = the
        positions of the layer's INPUT layout (segp), K axis = the slots of its OUTPUT layout"""
        blk = m["blk"]
        which = "Minv" if m["prim"] == "affine_bwd" else "M"
        out_phys = self._phys(self.natp_idx if m["out_layout"] == "natp" else self.segp_idx)
        return self._planes_image(pk, ("pl_aff_t", id(blk), which, m["out_layout"]), self._affine_entry(pk, blk)[which],
                                  self.segp_idx, out_phys, _ext.PLANES_BF16X3, transpose=True)

    def planes_coupling_bwd(self, pk, m) -> dict:
        """the backward image set of the coupling whose ``meta`` entry is m (_coupling_planes_images), kept with the layer"""
        cp = pk["coupling"][m["step"]]
        if "planes_bwd" not in cp:
            cp["planes_bwd"] = self._coupling_planes_images(pk, m["step"], m, _ext.PLANES_BF16X3, backward=True)
        return cp["planes_bwd"]

    def planes_coupling_bwd_op(self, pk, m, g, g_nkb: int, B: int, gates, d_out) -> _ext.Op:
        """ONE launch for the data-gradient chain of a coupling layer's conditioner on the gradient planes buffer g:
        g[:, conditioning blocks] += sign * MLP^T(g[:, transformed blocks]); gates / d_out: planes buffers (8 blocks per panel)
        in the FORWARD's layer order -- the saved activations resp. the gradients at the pre-activations"""
        cp = pk["coupling"][m["step"]]
        return coupling_planes_op(g, g_nkb, B, (m["kb_t0"], m["nk_t"], m["kb_p0"], m["nk_p"]),      # the roles of the block ranges swap
                                  self.planes_coupling_bwd(pk, m), m["sign"], cp["slope"], _ext.ACT_GATE, _ext.PLANES_BF16X3, 0,
                                  gate=gates[::-1], hidden_out=d_out[::-1])

    def _build_plan_planes(self, direction: str, B: int, device, final: str, train: bool = False, has_ctx: bool = False) -> dict:
        """Launch list of the planes pipeline: pack -> (GEMM on planes)* -> GEMM with fp32 output.

        Every layer is the same kernel: an affine block one GEMM, an additive coupling the chain of its conditioner's
        dense layers (the hidden activations make a round trip through HBM / the Infinity Cache as planes; the last
        one adds / subtracts into the transformed half of z IN PLACE, reading the residual from the planes).  The
        buffer z keeps the engine's segment layout [mask==0 | mask==1] padded to whole 32-feature blocks; a coupling
        reads the blocks that hold its conditioning features (zero weights on the others) and rewrites the blocks
        that hold its transformed features (zero rows elsewhere: those values are rewritten unchanged)."""
        p = _PlanesPlan(self, direction, B, device, final, train, has_ctx)
        k = p.head()
        while k < len(p.prims):
            prim, i = p.prims[k]
            k += p.affine(k, prim, i) if prim in ("affine_fwd", "affine_bwd") else p.coupling(prim, i)
        return p.result()


def coupling_planes_op(z, z_nkb: int, B: int, ranges, f: dict, sign, slope, act, fmt, flag, gate=(), hidden_out=()) -> _ext.Op:
    """THE filler of the ``coupling_planes`` descriptor: the planes buffer z (z_nkb blocks per panel, B rows), the block ranges
    (kb_p0, nk_p, kb_t0, nk_t), an image set f (PlanesPlanMixin._coupling_planes_images), and per hidden layer the optional
    planes buffers of the gates (USF_ACT_GATE) / the hidden side outputs"""
    op = _ext.Op()
    op.kind = _ext.OP_COUPLING_PLANES
    c = op.u.coupling_planes
    c.z, c.z_nkb, c.M = z.data_ptr(), z_nkb, B
    c.kb_p0, c.nk_p, c.kb_t0, c.nk_t = ranges
    c.n_hidden, c.hidden_padded = len(f["hid"]) + 1, 256
    c.W_in, c.ldw_in, c.w_in_plane = _image_triple(f["W_in"])
    c.b_in = f["b_in"].data_ptr()
    for j, (Wh, bh) in enumerate(zip(f["hid"], f["b_hid"])):
        c.W_hid[j], c.ldw_hid, c.w_hid_plane = _image_triple(Wh)
        c.b_hid[j] = bh.data_ptr()
    c.W_out, c.ldw_out, c.w_out_plane = _image_triple(f["W_out"])
    c.b_out = f["b_out"].data_ptr()
    c.sign, c.slope, c.act, c.format, c.range_flag = sign, slope, act, fmt, flag
    for l, t in enumerate(gate):
        c.gate[l] = t.data_ptr()
    for l, t in enumerate(hidden_out):
        c.hidden_out[l] = t.data_ptr()
    return op


class _PlanesPlan:
    """A planes plan under construction (PlanesPlanMixin._build_plan_planes): the op list and its bookkeeping, the planes
    buffer the next layer reads (``z``) and the one an affine layer writes (``other``), and one method per kind of layer."""

    def __init__(self, eng, direction: str, B: int, device, final: str, train: bool, has_ctx: bool):
        self.eng, self.B, self.device, self.final, self.train, self.has_ctx = eng, B, device, final, train, has_ctx
        self.pk = eng.pack(device)
        ws = self.ws = eng._workspace(B, device)
        self.prims = eng._primitive_ops(direction, merge=not train)     # (the training backward needs every block's own launch)
        self.nkb = eng.LDp // 32
        self.seg_phys = eng._phys(eng.segp_idx)
        self.fmt = eng._planes_fmt()
        if "pflag" not in ws:
            ws["pflag"] = torch.zeros(1, dtype=torch.int32, device=device)
        self.flag = ws["pflag"].data_ptr() if self.fmt == _ext.PLANES_F16X2 else 0
        # training: every affine output keeps a planes buffer of its own (the saved activations of the backward pass,
        # already in operand form: (K + 1) x B x LDp x 6 bytes -- cfg2 at 65536 rows: 10.4 GB of the 288 GB), couplings update
        # theirs in place (their conditioning half -- all the backward needs of them -- is untouched)
        self.z_name, self.other_name = ("pz0", None) if train else ("pzA", "pzB")
        self.z = self.planes_buf(self.z_name, self.nkb)
        self.other = None if train else self.planes_buf(self.other_name, self.nkb)
        self.n_z = 1
        self.ops: List[_ext.Op] = []
        self.meta: List[dict] = []
        self.patch_in, self.patch_out = [], []
        self.head_scale, self.bias_in_head, self.out_buf = None, False, None
        self.side_for = None            # (coupling step, nk_t) whose residual the last affine GEMM left as fp32 (_side_output)

    def planes_buf(self, name: str, blocks: int) -> torch.Tensor:
        ws, n = self.ws, (-(-self.B // 16)) * blocks * 3072            # (sized for either format)
        if name not in ws or ws[name].numel() < n:
            ws[name] = torch.empty(n, dtype=torch.uint8, device=self.device)
        return ws[name]

    def gemm_op(self, W: torch.Tensor, **kw) -> _ext.Op:
        """a usf_gemm_planes op on the weight image W; kw: the descriptor fields that differ from the plain product"""
        op = _ext.Op()
        op.kind = _ext.OP_GEMM_PLANES
        g = op.u.gemm_planes
        g.M, g.res_sign, g.slope, g.act = self.B, 1.0, 0.0, _ext.ACT_NONE
        g.format, g.range_flag = self.fmt, self.flag
        g.W_planes, g.ldw, g.w_plane_stride = _image_triple(W)
        g.w_rows = W.shape[1]
        for k_, v_ in kw.items():
            setattr(g, k_, v_)
        return op

    def head(self) -> int:
        """the caller's fp32 rows -> planes in segment layout (+ x / s - b of the first layer); returns how many primitives
        the pack op took"""
        e, pk, prims = self.eng, self.pk, self.prims
        segp = e.segp_idx
        pack = _ext.Op()
        pack.kind = _ext.OP_PACK_PLANES
        d = pack.u.pack_planes
        d.src, d.ld, d.M, d.nkb = 0, e.D, self.B, self.nkb
        d.src_cols = e.D                    # (every index of the layout is a feature number: rows are read whole, coalesced)
        d.format, d.range_flag = self.fmt, self.flag
        d.idx = e._idx_dev("segp", self.device).data_ptr()
        d.planes = self.z.data_ptr()
        k = 0
        if prims[0][0] == "scale_div":
            self.head_scale = s0 = e._step(prims[0][1]).module
            d.pre_div = e._planes_vec(pk, ("pl_scale", id(s0), "segp"), pk["scale"][id(s0)], segp, 1.0).data_ptr()
            if prims[1][0] == "affine_bwd":      # (x / s - b) Minv^T: the bias goes into the head as well
                blk = e._step(prims[1][1]).module
                d.pre_sub = e._planes_vec(pk, ("pl_b", id(blk), "segp"), pk["affine"][id(blk)]["b"], segp).data_ptr()
                self.bias_in_head = True
            k = 1
        self.patch_in.append((len(self.ops), "pack_planes", "src"))
        self.ops.append(pack)
        return k

    def affine(self, k: int, prim: str, i: int) -> int:
        """an affine block (with the flow's last ScaleTransform in its epilogue): ONE GEMM, planes -> planes, or -> the fp32
        result when it is the last layer; returns how many primitives it took"""
        e, pk, nkb = self.eng, self.pk, self.nkb
        blk = e._step(i).module
        a = e._affine_entry(pk, blk)
        fuse_post, is_last, taken = affine_span(self.prims, k)      # (_planes_ok admits a scale_mul at the very end only)
        is_head = len(self.ops) == 1                    # the first layer behind the pack op: the head's prologue belongs to it
        lay, out_sel = ("natp", e.natp_idx) if is_last else ("segp", e.segp_idx)
        if self.train:
            self.meta.append(dict(kind="affine", op=len(self.ops), prim=prim, blk=blk, in_buf=self.z_name, in_layout="segp",
                                  out_layout=lay, N=e.D if is_last else e.LD, K=e.LD,
                                  pre_scale=self.head_scale if is_head else None, post_scale=None,
                                  pre_sub_folded=bool(is_head and self.bias_in_head), is_last=is_last))
        which = "Minv" if prim == "affine_bwd" else "M"
        W = e._planes_image(pk, ("pl_aff", id(blk), which, is_last), a[which], out_sel, self.seg_phys, self.fmt)
        kw = dict(A=self.z.data_ptr(), a_nkb=nkb, a_kb0=0, nk=nkb)
        if prim == "affine_fwd":
            kw["bias"] = e._planes_vec(pk, ("pl_b", id(blk), lay), a["b"], out_sel).data_ptr()
        elif not (is_head and self.bias_in_head):       # (x / s - b) @ Minv^T: bias already subtracted by the head
            kw["bias"] = e._planes_vec(pk, ("pl_c", id(blk), lay), folded_bias(a), out_sel).data_ptr()
        if is_last:
            if fuse_post:
                s2 = e._step(self.prims[k + 1][1]).module
                kw["post_mul"] = e._planes_vec(pk, ("pl_scale", id(s2), "natp"), pk["scale"][id(s2)], e.natp_idx, 1.0).data_ptr()
            self._final_store(kw)
        else:
            if self.train:
                self.other_name = f"pz{self.n_z}"
                self.other = self.planes_buf(self.other_name, nkb)
                self.n_z += 1
            kw.update(C_planes=self.other.data_ptr(), c_nkb=nkb, c_kb0=0, c_kbn=nkb)
            self.z, self.z_name, self.other, self.other_name = self.other, self.other_name, self.z, self.z_name
            self._side_output(k + taken)
        if self.train:
            self.meta[-1]["out_buf"] = self.out_buf[0] if is_last else self.z_name
        self.ops.append(self.gemm_op(W, **kw))
        return taken

    def side_range(self, k: int):
        """the fp32 side output of the affine GEMM in front of primitive k: None, or (coupling step, kb_t0, nk_t, both_kb0,
        both_kbn) when that primitive is a coupling of this plan that runs as ONE fused launch without a context -- the only
        reader of the transformed blocks [kb_t0, kb_t0 + nk_t) of the GEMM's output then wants them as fp32 (its residual).  The
        blocks of that range which also hold conditioning features (both) are written as planes as well: the coupling's first
        layer reads them.  Inference plans from planes_side_min_rows rows, knob planes_side_f32."""
        e = self.eng
        if self.train or not e.planes_side_f32 or self.B < e.planes_side_min_rows or k >= len(self.prims):
            return None
        prim, i = self.prims[k]
        if prim not in ("coupling_fwd", "coupling_bwd"):
            return None
        cp = self.pk["coupling"][i]
        if (self.has_ctx and cp["has_ctx"]) or not e._planes_coupling_fused(list(cp["raw"]["h"]), self.B, self.fmt):
            return None
        geo = e._coupling_geometry(cp)
        t0, t1 = geo["kb_t0"], geo["kb_t0"] + geo["nk_t"]
        b0, b1 = max(t0, geo["kb_p0"]), min(t1, geo["kb_p0"] + geo["nk_p"])
        return (i, t0, t1 - t0, b0, b1 - b0) if b1 > b0 else (i, t0, t1 - t0, t0, 0)

    def _side_output(self, k: int) -> None:
        """the prefix op in front of an affine GEMM whose transformed half goes to the coupling behind it as fp32 (side_range)"""
        self.side_for = None
        r = self.side_range(k)
        if r is None:
            return
        i, t0, nt, b0, nb = r
        # ONE buffer per plan, reused by every (GEMM, coupling) pair: sized for the widest transformed range of the flow's
        # couplings up front (ops built earlier hold its address)
        ws = self.ws
        nmax = max(self.eng._coupling_geometry(cp)["nk_t"] for cp in self.pk["coupling"].values())
        n = (-(-self.B // 16)) * nmax * 2048
        if "pside" not in ws or ws["pside"].numel() < n:
            ws["pside"] = torch.empty(n, dtype=torch.uint8, device=self.device)
        self.ops.append(_ext.gemm_planes_side_prefix(ws["pside"], t0, nt, b0, nb))
        self.side_for = (i, nt)

    def _final_store(self, kw: dict) -> None:
        """where the last GEMM's fp32 result goes (``final``): sets its descriptor fields in kw and ``out_buf``"""
        e, ws, B, final = self.eng, self.ws, self.B, self.final
        if final == "user":
            kw.update(C_f32=0, ldc=e.D, N=e.D)
            self.patch_out.append((len(self.ops), "gemm_planes", "C_f32"))
            self.out_buf = ("user_out", "nat", e.D)
        elif final.startswith("base"):
            # Flow.log_prob: z only feeds the base density -- the epilogue reduces the row's Laplace / Normal terms per
            # column block ([B, 8] partial sums; tables refreshed per call by Engine.latent) and stores no rows
            stride = _round_up(e.D, 4)
            if "btab" not in ws:
                ws["btab"] = torch.zeros(3 * stride, dtype=torch.float32, device=self.device)
                ws["bpart"] = torch.zeros(B, 8, dtype=torch.float32, device=self.device)
            kw.update(C_f32=0, ldc=e.D, N=e.D, base_tab=ws["btab"].data_ptr(), base_tab_stride=stride,
                      base_part=ws["bpart"].data_ptr(), base=int(final[4:]))
            self.out_buf = ("bpart", "part", 8)
        else:
            kw.update(C_f32=e._nat2(ws, B, self.device).data_ptr(), ldc=e.LDn, N=e.D)
            self.out_buf = ("nat2", "nat", e.LDn)

    def coupling(self, prim: str, i: int) -> int:
        """an additive coupling, in place on the transformed blocks of z: ONE fused launch, or its conditioner as a chain of GEMMs"""
        e = self.eng
        cp = self.pk["coupling"][i]
        geo = e._coupling_geometry(cp)
        sign = 1.0 if prim == "coupling_fwd" else -1.0
        use_ctx = bool(self.has_ctx and cp["has_ctx"])
        if e._planes_coupling_fused(list(cp["raw"]["h"]), self.B, self.fmt):
            self._coupling_fused(i, cp, geo, sign, use_ctx)
        elif self.train or use_ctx:
            raise EngineUnsupported("training / a context on the planes pipeline needs the fused coupling launch")
        else:
            self._coupling_chained(i, cp, geo, sign)
        return 1

    def _coupling_fused(self, i: int, cp: dict, geo: dict, sign: float, use_ctx: bool) -> None:
        """ONE launch per layer: usf_coupling_planes (hidden activations stay in registers; widths padded to 256)"""
        e, pk, ws = self.eng, self.pk, self.ws
        raw = cp["raw"]
        f = e._coupling_planes_images(pk, i, geo, self.fmt)
        if use_ctx:
            # ConditionalDenseNN's context layer (context_dim 1): the launch becomes usf_coupling_planes_ctx -- a prefix
            # op hands the coupling op behind it ws["ctx"] and layers[1]'s weight column / bias as 256-wide vectors
            Wc, bc = raw["ctx"]
            rows0 = arange_padded(raw["h"][0], 256)
            w_ctx = e._planes_vec(pk, ("pl_cctxw", i), Wc, rows0)
            b_ctx = e._planes_vec(pk, ("pl_cctxb", i), bc, rows0)
            self.ops.append(_ext.coupling_planes_ctx_prefix(ws["ctx"], 1, w_ctx, b_ctx))
        # training: the lane-local splits of the hidden activations also go to planes buffers of the layer's own (8 blocks:
        # 2 x B x 256 x 6 bytes per coupling): operands of the conditioner's weight gradients, gates of its backward
        hnames = [f"pHs{j}_{i}" for j in range(len(raw["h"]))] if self.train else []
        op = coupling_planes_op(self.z, self.nkb, self.B, (geo["kb_p0"], geo["nk_p"], geo["kb_t0"], geo["nk_t"]), f, sign,
                                cp["slope"], cp["act"], self.fmt, self.flag, hidden_out=[self.planes_buf(hn, 8) for hn in hnames])
        if self.train:
            self.meta.append(dict(kind="coupling", op=len(self.ops), step=i, buf=self.z_name, sign=sign, use_ctx=use_ctx,
                                  hidden_planes=hnames, **geo))
        if self.side_for == (i, geo["nk_t"]) and not use_ctx:
            # the affine GEMM in front of the layer left the transformed half as fp32 (_side_output): the residual comes from there
            self.ops.append(_ext.coupling_planes_side_prefix(ws["pside"], geo["nk_t"]))
        self.side_for = None
        self.ops.append(op)

    def _coupling_chained(self, i: int, cp: dict, geo: dict, sign: float) -> None:
        """the conditioner MLP as a chain of GEMMs through a pair of hidden planes buffers; the last one adds into z"""
        e, pk, z, nkb = self.eng, self.pk, self.z, self.nkb
        raw = cp["raw"]
        h = list(raw["h"])
        layers = [raw["first"]] + list(raw["hidden"]) + [raw["last"]]
        hkb = _round_up(e.hmax, 32) // 32
        hbufs = [self.planes_buf("pH1", hkb), self.planes_buf("pH2", hkb)]
        src = dict(A=z.data_ptr(), a_nkb=nkb, a_kb0=geo["kb_p0"], nk=geo["nk_p"])
        in_sel = geo["feat_p"][32 * geo["kb_p0"]: 32 * (geo["kb_p0"] + geo["nk_p"])]
        for j, (W_, b_) in enumerate(layers):
            last = j == len(layers) - 1
            if last:
                out_sel = geo["feat_t"][32 * geo["kb_t0"]: 32 * (geo["kb_t0"] + geo["nk_t"])]
                dst = dict(C_planes=z.data_ptr(), c_nkb=nkb, c_kb0=geo["kb_t0"], c_kbn=geo["nk_t"], residual=z.data_ptr(), res_sign=sign)
            else:
                hj = _round_up(h[j], 32)
                out_sel = arange_padded(h[j], hj)
                buf = hbufs[j % 2]
                dst = dict(C_planes=buf.data_ptr(), c_nkb=hkb, c_kb0=0, c_kbn=hj // 32, act=cp["act"], slope=cp["slope"])
            Wimg = e._planes_image(pk, ("pl_mlp", i, j), W_, out_sel, e._phys(in_sel), self.fmt)
            bvec = e._planes_vec(pk, ("pl_mlpb", i, j), b_, out_sel)
            self.ops.append(self.gemm_op(Wimg, bias=bvec.data_ptr(), **src, **dst))
            if not last:
                src, in_sel = dict(A=buf.data_ptr(), a_nkb=hkb, a_kb0=0, nk=hj // 32), out_sel

    def result(self) -> dict:
        ops, out_buf = self.ops, self.out_buf
        arr = (_ext.Op * len(ops))(*ops)
        n_part = 0
        if out_buf[1] == "part":
            tn = (_ext.load().usf_gemm_planes_variant(arr[len(ops) - 1].u.gemm_planes) - 5000) // 10
            n_part = -(-self.eng.D // (32 * tn))
        return dict(arr=arr, n=len(ops), patch_in=self.patch_in, patch_out=self.patch_out, side=[], final_gather=None,
                    n_part=n_part, out_buf=out_buf, ws=self.ws, pk=self.pk, meta=self.meta, planes=True, planes_fmt=self.fmt,
                    planes_train=bool(self.train), has_ctx=bool(self.has_ctx))
