"""The fp32-row plans: between layers the activations are fp32 rows in the segment layout -- the op lists of
every small batch, of ``gemm_mode = "f32"``, of general (gated / layer-norm) conditioners and vector contexts, and of the
fp32-row training step (``usf_linear_f32``, the fused coupling kernels, ``usf_gated_norm_rows_f32``), and the conditioner weight
images they read.  A mixin of ``usflows_amd.engine.FlowEngine``, the counterpart of engine_planes.py."""
from __future__ import annotations

import ctypes as C
from typing import List

import torch

from . import _ext
from .config import config
from ._plan_util import _image_triple, _round_up, affine_span, folded_bias, kperm


class FlatPlanMixin:
    """see the module docstring"""

    # ---- conditioner weight images: the chain-of-linears form ---------------------------------------------------------------
    def _unfused_pack(self, pk, cp) -> dict:
        """per-layer weight images for the chain-of-linears form of the conditioner (any width / depth)"""
        if "unfused" in cp:
            return cp["unfused"]
        with self._pk_record(pk):
            return self._unfused_pack_build(cp)

    def _unfused_pack_build(self, cp) -> dict:
        raw = cp["raw"]
        dev, h, hp = raw["device"], raw["h"], cp["hidden"]
        pass_sel = self._sel(raw["pass_idx"], cp["pass_n"], dev)
        layers = []
        mats = self._pack["mats"]

        def image(src, out_sel, n_out, in_sel, n_in):
            """fp32 image + (when the linear kernel will take the bf16x3 path for it) its planes, both from `src`"""
            pl = _round_up(n_in, 32) if self._wants_planes(n_out, n_in) else 0
            Wp, P = self._packed(src, out_sel, n_out, in_sel, n_in, planes_ld=pl)
            if P is not None:
                mats[("planes", Wp.data_ptr())] = P
            mats[("imgsrc", Wp.data_ptr())] = (src, out_sel, n_out, in_sel, n_in)      # for the transposed image
            return Wp

        if cp.get("general"):
            return self._general_pack_build(cp, image, pass_sel)
        W, b = raw["first"]
        Wp = image(W, self._iarange(h[0], hp[0], dev), hp[0], pass_sel, cp["pass_n"])
        layers.append((Wp, self._packed_vec(b, self._iarange(h[0], hp[0], dev), hp[0])))
        for j, (W, b) in enumerate(raw["hidden"]):
            Wp = image(W, self._iarange(h[j + 1], hp[j + 1], dev), hp[j + 1], self._iarange(h[j], hp[j], dev), hp[j])
            layers.append((Wp, self._packed_vec(b, self._iarange(h[j + 1], hp[j + 1], dev), hp[j + 1])))
        W, b = raw["last"]
        tr_sel = self._sel(raw["tr_idx"], cp["tr_n"], dev)
        W_out = image(W, tr_sel, cp["tr_n"], self._iarange(h[-1], hp[-1], dev), hp[-1])
        u = dict(layers=layers, W_out=W_out, b_out=self._packed_vec(b, tr_sel, cp["tr_n"]))
        if cp["has_ctx"]:
            Wc, bc = raw["ctx"]
            rows = self._iarange(h[0], hp[0], dev)
            # [h0, Cp]: the context rides in columns [0, C) of a K padded to a multiple of 4 (C = 1: column 0 of a 4-wide K)
            Cp = _round_up(self.ctx_dim, 4)
            u["W_ctx4"], _ = self._packed(Wc, rows, hp[0], self._iarange(self.ctx_dim, Cp, dev), Cp)
            u["b_ctx"] = self._packed_vec(bc, rows, hp[0])
        cp["unfused"] = u
        return u

    def _general_pack_build(self, cp, image, pass_sel) -> dict:
        """weight images of a vector ConvNet conditioner with GatedMLP / LayerNormVector blocks: every Linear padded to
        multiples of 4 with zeros; a GatedMLP's second Linear keeps its value rows in [0, wp) and its gate rows in
        [wp, 2 wp) (wp = padded block width), so ``chunk(2, dim=1)`` is two column offsets"""
        raw = cp["raw"]
        dev = raw["device"]
        r4 = lambda n: _round_up(n, 4)      # noqa: E731
        ar = lambda n: self._iarange(n, r4(n), dev)      # noqa: E731
        tensors = []

        def lin(Wb, out_sel, n_out, in_sel, n_in):
            W, b = Wb
            Wp = image(W, out_sel, n_out, in_sel, n_in)
            bp = self._packed_vec(b, out_sel, n_out)
            tensors.extend([Wp, bp])
            return Wp, bp

        h0 = raw["h"][0]
        u = dict(general=True, first=lin(raw["first"], ar(h0), r4(h0), pass_sel, cp["pass_n"]), blocks=[])
        for b in raw["blocks"]:
            wi, wo = b["w_in"], b["w_out"]
            e = dict(w_in=wi, w_out=wo, eps=b["eps"])
            if "lin" in b:
                e["lin"] = lin(b["lin"], ar(wo), r4(wo), ar(wi), r4(wi))
            else:
                e["l1"] = lin(b["l1"], ar(wo), r4(wo), ar(wi), r4(wi))
                two = torch.full((2 * r4(wo),), -1, dtype=torch.int32)
                two[:wo] = torch.arange(wo, dtype=torch.int32)
                two[r4(wo): r4(wo) + wo] = torch.arange(wo, 2 * wo, dtype=torch.int32)
                e["l2"] = lin(b["l2"], two.to(dev), 2 * r4(wo), ar(wo), r4(wo))
                if "proj" in b:
                    e["proj"] = lin(b["proj"], ar(wo), r4(wo), ar(wi), r4(wi))
            if "ln" in b:
                g_, b_ = b["ln"]
                e["ln"] = (self._packed_vec(g_, ar(wo), r4(wo)), self._packed_vec(b_, ar(wo), r4(wo)))
                tensors.extend(e["ln"])
            u["blocks"].append(e)
        w_last = raw["blocks"][-1]["w_out"]
        tr_sel = self._sel(raw["tr_idx"], cp["tr_n"], dev)
        u["W_out"], u["b_out"] = lin(raw["last"], tr_sel, cp["tr_n"], ar(w_last), r4(w_last))
        u["tensors"] = tensors
        cp["unfused"] = u
        return u

    # ---- which kernel serves a coupling, and what a training plan keeps of it -----------------------------------------------
    def tiny_coupling(self, cp, B: int) -> bool:
        """launch-bound batches with tiny conditioners (the reference's live flat configuration, gaussian_mixture.yaml: D <= 100,
        DenseNN [32, 32], batch 32): the whole coupling layer is one launch of the tiny-layer kernel each way
        (usf_coupling_tiny.hip's eligibility rule, restated for the forward AND the backward descriptor: <= 256 rows, segments
        and hidden widths <= 64, the layer's weight images + rows + side inputs in 64 KB of LDS)"""
        if not config.tiny_coupling or not config.get_lib("coupling_tiny", 1) or not (0 < B <= 256) or cp.get("general"):
            return False
        hid = [int(h_) for h_ in cp["hidden"]]
        if len(hid) > 3 or max(hid) > 64 or cp["pass_n"] > 64 or cp["tr_n"] > 64:
            return False

        def lds_floats(n_pass, hidden, n_trans):
            r4 = lambda v: (v + 3) // 4 * 4
            f, k, rows_sum = 0, n_pass, 0
            for rows in list(hidden) + [n_trans]:
                f += (rows + 15) // 16 * 16 * (r4(k) + 4)
                rows_sum += rows
                k = rows
            return f + 32 * (r4(n_pass) + 4) + 2 * 32 * 68 + rows_sum + 32 * n_trans + 32 * sum(hidden) + 32 + 128

        return max(lds_floats(cp["pass_n"], hid, cp["tr_n"]), lds_floats(cp["tr_n"], hid[::-1], cp["pass_n"])) * 4 <= 64 * 1024

    def _hidden_bufs(self, ws, i, n, B, device):
        """the buffers ``Hs{j}_{i}`` [B, hmax] a training plan's coupling step i keeps its n hidden activations in -- whichever
        forward wrote them (the unfused chain's GEMMs, the fused kernels' ``hidden_out``); the training backward asks here too"""
        for j in range(n):
            hname = f"Hs{j}_{i}"
            if hname not in ws or ws[hname].shape[0] != B or ws[hname].shape[1] < self.hmax:
                ws[hname] = torch.zeros(B, self.hmax, dtype=torch.float32, device=device)
        return [ws[f"Hs{j}_{i}"] for j in range(n)]

    def _tiny_served(self, pk, cp, op, ws, i, B, train, device, ctx_dim: int = 0) -> bool:
        """the library's own answer for a layer tiny_coupling() admits: the tiny-layer kernel serves the forward descriptor and,
        for a training plan whose backward chain runs fused (training_rows.py: fused_cbwd), the backward one (usf_coupling_variant,
        host-only).  Otherwise the layer takes the unfused ops: the f32 kernel rejects hidden_out / GATE"""
        lib = _ext.load()
        # (a vector context's LDS segments count against the kernel's budget: usf_coupling_additive_vctx_variant knows)
        if (_ext.coupling_vctx_variant(op, ctx_dim) if ctx_dim else lib.usf_coupling_variant(C.byref(op.u.coupling))) != 3:
            return False
        if train and config.fused_cbwd:
            hb = self._hidden_bufs(ws, i, len(cp["hidden"]), B, device)
            bop = self.coupling_backward_op(pk, cp, op.u.coupling.z, self.LD, B, 1.0, hb, hb)
            if lib.usf_coupling_variant(C.byref(bop.u.coupling)) != 3:
                return False
        return True

    def save_fused_hidden(self, cp, B: int) -> bool:
        """training: the fused bf16x3 coupling kernel stores its hidden activations (usf_coupling_desc::hidden_out) -- where
        that kernel serves the layer (hidden width in (128, 256], >= 1024 rows, a row buffer whose element offsets fit 32 bits:
        coupling_bf16x3_eligible's rule M * ldz < 2^32, restated for the forward launch on the [B, LD] rows and the backward
        launch on the gradient rows, [B, LD] or [B, LDn]), unless USFLOWS_AMD_SAVE_HIDDEN=0"""
        hm = max(cp["hidden"])
        return (self.gemm_mode == "bf16x3" and config.save_hidden and 128 < hm <= 256
                and B >= 1024 and B * max(self.LD, self.LDn) < (1 << 32) and self.hmax >= 256 and self.hmax % 4 == 0
                and cp["tr_n"] % 4 == 0 and cp["tr_off"] % 4 == 0)      # (the backward launch reads the transformed half as its input)

    def wgrad_from_planes(self, B: int, N: int, K: int) -> bool:
        """weight gradients of the training step from pre-split operand planes (usf_wgrad_planes_f32): in the bf16x3 mode,
        where the kernel pays (its own cross-over), unless USFLOWS_AMD_WGRAD_PLANES=0"""
        rows, wid = -(-B // 32) * 32, -(-max(N, K, self.LD, self.LDn) // 32) * 32
        return (self.gemm_mode == "bf16x3" and config.wgrad_planes
                and 3 * rows * wid * 2 < (1 << 31)          # the three planes of an operand stay below 2 GiB (32-bit offsets)
                and _ext.wgrad_planes_ok(B, N, K))

    # fused coupling kernel availability (filled in when the kernel is present)
    def _fused_ok(self, cp) -> bool:
        lib = _ext.load()
        wmax = lib.usf_coupling_max_width()
        return not cp.get("general") and wmax > 0 and len(cp["hidden"]) <= 3 and max(cp["hidden"]) <= wmax

    def _fused_pack(self, cp) -> dict:
        """weights re-laid out for the fused kernel's padding contract (include/usflows_hip.h)"""
        Hp = _ext.load().usf_coupling_padded_width(max(cp["hidden"]))
        split = self.gemm_mode in ("bf16x3", "f16x2") and Hp == 256
        if "fused" in cp and (not split or "split" in cp["fused"]):
            return cp["fused"]
        with self._pk_record(self._pack):
            cp["fused"] = self._fused_images(cp, Hp, split)
        return cp["fused"]

    def _fused_pack_bwd(self, pk, cp) -> dict:
        """the conditioner's weights transposed and re-laid out for the fused kernel run BACKWARDS (usf_coupling_desc::gate):
        W_in = W_last^T [hidden, trans], hidden matrices reversed and transposed, W_out = W_first^T [pass, hidden], zero biases"""
        if "fused_bwd" not in cp:
            Hp = _ext.load().usf_coupling_padded_width(max(cp["hidden"]))
            with self._pk_record(pk):
                cp["fused_bwd"] = self._fused_images(cp, Hp, True, backward=True)
        return cp["fused_bwd"]

    def _fused_images(self, cp, Hp: int, split: bool, backward: bool = False) -> dict:
        """the fused kernel's image set in one direction: W_in / hid [(W, b)] / W_out with their biases (backward: one shared zero
        vector, and the roles of the column segments swap), and with ``split`` the bf16x3 planes of every matrix"""
        raw = cp["raw"]
        dev, h = raw["device"], raw["h"]
        layers = [raw["first"]] + list(raw["hidden"]) + [raw["last"]]
        n = len(layers)
        # the index set (and its padded width) at both ends of every layer: layer j maps ends[j] -> ends[j + 1]
        wid = [_round_up(cp["pass_n"], 32)] + [Hp] * len(h) + [_round_up(cp["tr_n"], 32)]
        ends = ([self._sel(raw["pass_idx"], wid[0], dev)] + [self._iarange(w, Hp, dev) for w in h]
                + [self._sel(raw["tr_idx"], wid[-1], dev)])
        zeros = torch.zeros(max(Hp, wid[0]), dtype=torch.float32, device=dev) if backward else None
        mats, planes, vecs = [], [], []
        for at, j in enumerate(reversed(range(n)) if backward else range(n)):
            o, k = (j, j + 1) if backward else (j + 1, j)           # the ends on the image's rows / on its K axis
            # hidden (K) axes of the split hidden / output planes in the accumulator order of the kernel
            psel = kperm(h[k - 1], Hp, dev) if (split and at > 0) else None
            W, P = self._packed(layers[j][0], ends[o], wid[o], ends[k], wid[k], planes_sel=psel, planes_ld=wid[k] if split else 0,
                                transpose=backward)
            mats.append(W)
            planes.append(P)
            vecs.append(zeros if backward else self._packed_vec(layers[j][1], ends[o], wid[o]))
        f = dict(Hp=Hp, W_in=mats[0], b_in=vecs[0], hid=list(zip(mats[1:-1], vecs[1:-1])), W_out=mats[-1], b_out=vecs[-1])
        if split:
            f["split"] = dict(hid=planes[1:-1])
            f["split"]["in"], f["split"]["out"] = planes[0], planes[-1]
        if backward:
            f["zeros"] = zeros
        elif cp["has_ctx"]:
            Wc, bc = raw["ctx"]
            if self.ctx_dim == 1:
                f["W_ctx"] = self._packed_vec(Wc, ends[1], Hp)        # layers[1].weight is [h0, 1]: one column
            else:
                # layers[1].weight [h0, C] TRANSPOSED to [C, Hp] rows (usf_coupling_additive_vctx_f32: a lane's four hidden
                # units are one 16-byte load per context column), zeros beyond h0
                f["W_ctx_t"], _ = self._packed(Wc, self._iarange(self.ctx_dim, self.ctx_dim, dev), self.ctx_dim, ends[1], Hp,
                                               transpose=True)
            f["b_ctx"] = self._packed_vec(bc, ends[1], Hp)
        return f

    def _fused_op(self, cp, f, zptr, ld, B, sign, act, backward: bool = False, split: bool = True) -> _ext.Op:
        """the ``coupling`` descriptor on the image set f (_fused_images), in place on the rows at zptr: segments and hidden
        widths (backward: swapped / reversed), the plain weight fields and, with ``split``, the split-plane ones"""
        op = _ext.Op()
        op.kind = _ext.OP_COUPLING
        d = op.u.coupling
        d.z, d.ldz, d.out, d.ldo, d.M = zptr, ld, zptr, ld, B
        seg_p, seg_t = (cp["pass_off"], cp["pass_n"]), (cp["tr_off"], cp["tr_n"])
        (d.off_pass, d.n_pass), (d.off_trans, d.n_trans) = (seg_t, seg_p) if backward else (seg_p, seg_t)
        hidden = cp["hidden"][::-1] if backward else cp["hidden"]
        d.n_hidden = len(hidden)
        for j, hh in enumerate(hidden):
            d.hidden[j] = hh
        d.W_in, d.ldw_in, d.b_in = f["W_in"].data_ptr(), f["W_in"].shape[1], f["b_in"].data_ptr()
        for j, (W, b) in enumerate(f["hid"]):
            d.W_hid[j], d.b_hid[j], d.ldw_hid[j] = W.data_ptr(), b.data_ptr(), W.shape[1]
        d.W_out, d.ldw_out, d.b_out = f["W_out"].data_ptr(), f["W_out"].shape[1], f["b_out"].data_ptr()
        d.sign, d.slope, d.act = sign, cp["slope"], act
        if split:
            s3 = f["split"]
            d.split_in, d.split_in_ld, d.split_in_plane = _image_triple(s3["in"])
            for j, P in enumerate(s3["hid"]):
                d.split_hid[j], d.split_hid_ld, d.split_hid_plane = _image_triple(P)
            d.split_out, d.split_out_ld, d.split_out_plane = _image_triple(s3["out"])
        return op

    def coupling_backward_op(self, pk, cp, gptr, ld, B, sign, gates, d_out, act=_ext.ACT_GATE) -> _ext.Op:
        """ONE launch for the data-gradient chain of a coupling layer's conditioner: g[:, pass] += sign * MLP^T(g[:, trans]) with
        the (Leaky)ReLU backward from the saved activations `gates` (layer order of the forward); d_out[l] receives the gradient
        at hidden activation l (forward order)"""
        op = self._fused_op(cp, self._fused_pack_bwd(pk, cp), gptr, ld, B, sign, act, backward=True)
        d = op.u.coupling
        for j, (gt, do) in enumerate(zip(gates[::-1], d_out[::-1])):
            d.gate[j], d.hidden_out[j] = gt.data_ptr(), do.data_ptr()
        d.ld_gate, d.ld_hidden_out = gates[0].shape[1], d_out[0].shape[1]
        return op

    def _coupling_op(self, cp, zptr, B, sign, ws_ctx) -> _ext.Op:
        f = self._fused_pack(cp)
        op = self._fused_op(cp, f, zptr, self.LD, B, sign, cp["act"],
                            split=self.gemm_mode in ("bf16x3", "f16x2") and "split" in f)
        if ws_ctx is not None and self.ctx_dim == 1:           # (a vector context travels in a prefix op: _FlatPlan._coupling_fused)
            d = op.u.coupling
            d.context = ws_ctx["ctx"].data_ptr()
            d.W_ctx, d.b_ctx = f["W_ctx"].data_ptr(), f["b_ctx"].data_ptr()
        return op

    # ---- plan construction --------------------------------------------------------------------------------------------------
    def _build_plan_body(self, direction: str, B: int, device, has_ctx: bool, final: str, train: bool = False) -> dict:
        """final: 'user' (last op writes the caller's [B,D] tensor) or 'nat' (workspace buffer, for the tail).

        Returns the ctypes op array plus the few launches that are not usf_run_ops ops
        (layout gathers at the ends, stand-alone scale layers), each tagged with the op index
        before which it runs."""
        p = _FlatPlan(self, direction, B, device, has_ctx, final, train)
        k = 0
        while k < len(p.prims):
            kind = p.prims[k][0]
            if kind.startswith("affine") or p.scale_leads_affine(k):
                k += p.affine(k)
            else:
                k += p.scale(k) if kind.startswith("scale") else p.coupling(k)
        return p.result()


def linear_op(**kw) -> _ext.Op:
    """a ``linear`` op with the descriptor fields kw"""
    op = _ext.Op()
    op.kind = _ext.OP_LINEAR
    for k_, v_ in kw.items():
        setattr(op.u.linear, k_, v_)
    return op


def gated_norm_op(B: int, cp: dict, skip, C_: int, out, out_act, vg=None, gate_off=0, ln=None, eps=0.0) -> _ext.Op:
    """a ``gated_norm`` op (usf_gated_norm_rows_f32) over C_ columns of B rows: skip [+ value * sigmoid(gate) of vg] [-> layer
    norm ln = (gamma, beta)], written to ``out`` and, through the conditioner's activation, to ``out_act``"""
    op = _ext.Op()
    op.kind = _ext.OP_GATED_NORM
    g = op.u.gated_norm
    g.skip, g.ld_skip, g.M, g.C, g.c_pad = skip.data_ptr(), skip.shape[1], B, C_, _round_up(C_, 4)
    if vg is not None:
        g.vg, g.ld_vg, g.gate_off = vg.data_ptr(), vg.shape[1], gate_off
    if ln is not None:
        g.gamma, g.beta, g.eps = ln[0].data_ptr(), ln[1].data_ptr(), eps
    if out is not None:
        g.out, g.ld_out = out.data_ptr(), out.shape[1]
    if out_act is not None:
        g.out_act, g.ld_act, g.act, g.slope = out_act.data_ptr(), out_act.shape[1], cp["act"], cp["slope"]
    return op


class _FlatPlan:
    """An fp32-row plan under construction (FlatPlanMixin._build_plan_body): the op list and its bookkeeping, the launches that
    are no usf_run_ops ops (``side``), where the activations are right now (``cur``), and one method per kind of layer."""

    def __init__(self, eng, direction: str, B: int, device, has_ctx: bool, final: str, train: bool):
        self.eng, self.B, self.device, self.has_ctx, self.final, self.train = eng, B, device, has_ctx, final, train
        self.pk = eng.pack(device)
        self.ws = eng._workspace(B, device)
        self.prims = eng._primitive_ops(direction, merge=not train)     # (the training backward needs every block's own launch)
        self.ops: List[_ext.Op] = []
        self.patch_in: List[int] = []       # ops whose A is the caller's input tensor
        self.patch_out: List[int] = []      # ops whose C is the caller's output tensor
        self.side: List[tuple] = []         # ("gather", at, src_cur, dst_name, dst_layout) | ("scale", at, buf, ld, vec, divide, ncols)
        self.meta: List[dict] = []          # per group of ops: what the training backward needs (training.py)
        self.cur = ("user_in", "nat", eng.D)     # (buffer name, layout, row stride)
        self.free = ["zA", "zB"]
        self.n_act = 0

    def take(self) -> str:
        """the segment-layout buffer the next layer writes"""
        if not self.train:
            return self.free.pop(0)
        # training: every affine output keeps its own buffer (the saved activations of the backward
        # pass; (K+1) x B x LD x 4 bytes -- cfg2 at B = 65536: 6.8 GB of the 288 GB)
        name = f"act{self.n_act}"
        self.n_act += 1
        if name not in self.ws:
            self.ws[name] = torch.zeros(self.B, self.eng.LD, dtype=torch.float32, device=self.device)
        return name

    def release(self, name: str) -> None:
        if not self.train and name in ("zA", "zB") and name not in self.free:
            self.free.append(name)

    def gather(self, dst: str, layout: str, ld: int) -> None:
        """a column gather of the current activations into ws[dst], in front of the next op"""
        self.side.append(("gather", len(self.ops), self.cur, dst, layout))
        self.release(self.cur[0])
        self.cur = (dst, layout, ld)

    def scale_leads_affine(self, k: int) -> bool:
        """a ScaleTransform's division in front of an affine block rides in that block's prologue"""
        return self.prims[k][0] == "scale_div" and k + 1 < len(self.prims) and self.prims[k + 1][0].startswith("affine")

    def affine(self, k: int) -> int:
        """an affine block as ONE linear op, with a ScaleTransform on its outer side fused: the division in front of it in the
        prologue, the multiplication behind an ``affine_fwd`` in the epilogue; returns how many primitives it took"""
        e, pk, ws, ops, B = self.eng, self.pk, self.ws, self.ops, self.B
        if self.cur[0] == "user_in" and e.D % 4 != 0:
            # rows of the caller's tensor are not 16-B aligned: stage through a padded copy
            self.gather("nat", "nat", e.LDn)
        cur = self.cur
        in_layout = cur[1]
        kw = {}
        pre_scale = None
        if self.prims[k][0] == "scale_div":
            pre_scale = e._step(self.prims[k][1]).module
            kw["pre_div"] = e._vec(pk, ("scale", id(pre_scale)), pk["scale"][id(pre_scale)], in_layout, 1.0).data_ptr()
            k += 1
        prim, i = self.prims[k]
        blk = e._step(i).module
        a = e._affine_entry(pk, blk)
        fuse_post, is_last, taken = affine_span(self.prims, k)
        post_scale = e._step(self.prims[k + 1][1]).module if fuse_post else None
        out_layout = "nat" if is_last else "seg"
        Kdim = e.LD if in_layout == "seg" else e.LDn
        if prim == "affine_bwd":
            W = e._mat(pk, blk, "Minv", out_layout, in_layout)
            if pre_scale is not None:
                # first layer of log_prob: (x / s - b) @ Minv^T, prologue in the operand registers
                kw["pre_sub"] = e._vec(pk, ("b", id(blk)), a["b"], in_layout, 0.0).data_ptr()
            else:
                kw["bias"] = e._vec(pk, ("c", id(blk)), folded_bias(a), out_layout, 0.0).data_ptr()
        else:
            W = e._mat(pk, blk, "M", out_layout, in_layout)
            kw["bias"] = e._vec(pk, ("b", id(blk)), a["b"], out_layout, 0.0).data_ptr()
            if post_scale is not None:
                kw["post_mul"] = e._vec(pk, ("scale", id(post_scale)), pk["scale"][id(post_scale)], out_layout, 1.0).data_ptr()
        assert W.shape[1] == Kdim
        kw.update(e._split_kw(pk, W, Kdim))
        if out_layout == "seg":
            dst = self.take()
            Ndim, ldc, cptr = e.LD, e.LD, ws[dst].data_ptr()
        elif self.final == "user":
            dst, Ndim, ldc, cptr = "user_out", e.D, e.D, 0
        else:
            dst, Ndim, ldc, cptr = "nat2", e.D, e.LDn, e._nat2(ws, B, self.device).data_ptr()
        if cur[0] == "user_in":
            self.patch_in.append(len(ops))
        if dst == "user_out":
            self.patch_out.append(len(ops))
        # training at thousands of rows: the GEMM also writes the bf16 planes it makes of its input -- the operand
        # of this layer's weight gradient, already split (usf_wgrad_planes_f32; 3 x B x LD x 2 bytes per layer)
        in_planes = None
        if (self.train and cur[0] != "user_in" and "pre_div" not in kw and "pre_sub" not in kw
                and e.wgrad_from_planes(B, Ndim, Kdim)):
            in_planes = f"apl{len(ops)}"
            t = ws.get(in_planes)
            if t is None or t.shape[1] != -(-B // 32) * 32 or t.shape[2] != -(-Kdim // 32) * 32:
                t = ws[in_planes] = _ext.row_planes(B, Kdim, self.device)
            kw.update(A_planes_out=t.data_ptr(), ldp_out=t.shape[2], planes_out_stride=t.shape[1] * t.shape[2])
        self.meta.append(dict(kind="affine", op=len(ops), prim=prim, blk=blk, in_buf=cur[0], in_layout=in_layout,
                              in_ld=cur[2], out_buf=dst, out_layout=out_layout, out_ld=ldc, N=Ndim, K=Kdim,
                              pre_scale=pre_scale, post_scale=post_scale, in_planes=in_planes))
        ops.append(linear_op(A=(0 if cur[0] == "user_in" else ws[cur[0]].data_ptr()), lda=cur[2],
                             W=W.data_ptr(), ldw=W.shape[1], C=cptr, ldc=ldc, M=B, N=Ndim, K=Kdim,
                             res_sign=1.0, slope=0.0, act=_ext.ACT_NONE, **kw))
        self.release(cur[0])
        self.cur = (dst, out_layout, ldc)
        return taken + (pre_scale is not None)

    def scale(self, k: int) -> int:
        """a stand-alone scale layer: an elementwise launch, in place on a workspace buffer"""
        e, pk = self.eng, self.pk
        prim, i = self.prims[k]
        mod = e._step(i).module
        if self.cur[0] == "user_in":
            self.gather("nat", "nat", e.LDn)
        cur = self.cur
        sc = e._vec(pk, ("scale", id(mod)), pk["scale"][id(mod)], cur[1], 1.0)
        self.side.append(("scale", len(self.ops), cur[0], cur[2], sc, prim == "scale_div", e.LD if cur[1] == "seg" else e.LDn))
        return 1

    def coupling(self, k: int) -> int:
        """an additive coupling, in place on a segment-layout buffer: ONE fused launch where a fused kernel serves the layer at
        this batch, else its conditioner as a chain of linear ops"""
        e = self.eng
        prim, i = self.prims[k]
        if self.cur[1] != "seg" or self.cur[0] in ("user_in", "nat", "nat2"):
            self.gather(self.take(), "seg", e.LD)
        cp = self.pk["coupling"][i]
        sign = 1.0 if prim == "coupling_fwd" else -1.0
        zptr = self.ws[self.cur[0]].data_ptr()
        use_ctx = self.has_ctx and cp["has_ctx"]
        m = dict(kind="coupling", op=len(self.ops), step=i, buf=self.cur[0], sign=sign, use_ctx=use_ctx)
        self.meta.append(m)
        if cp.get("general"):
            self._coupling_general(cp, zptr, sign)
        elif not self._coupling_fused(m, cp, zptr, sign):
            self._coupling_unfused(m, cp, zptr, sign)
        return 1

    def _coupling_fused(self, m: dict, cp: dict, zptr: int, sign: float) -> bool:
        """ONE launch of a fused coupling kernel; False (and nothing laid out) where none serves the layer at this batch.
        The fused kernel keeps a wave on 16 rows for the whole MLP: unbeatable when the chip is full, but its latency is one
        wave's serial MFMA chain -- below ``fused_min_rows`` only layers the tiny-layer kernel takes run fused"""
        e, pk, ws, B, i = self.eng, self.pk, self.ws, self.B, m["step"]
        if not (e.use_fused_coupling and e._fused_ok(cp) and (B >= e.fused_min_rows or e.tiny_coupling(cp, B))):
            return False
        op = e._coupling_op(cp, zptr, B, sign, ws if m["use_ctx"] else None)
        vctx = m["use_ctx"] and e.ctx_dim > 1
        tiny = B < e.fused_min_rows
        if tiny and not e._tiny_served(pk, cp, op, ws, i, B, self.train, self.device, e.ctx_dim if vctx else 0):
            return False
        # training: the fused kernel also stores the hidden activations (buffers of the layer's own; 2 x B x 256 x 4
        # bytes per coupling) -- the backward pass reads them instead of running the conditioner a second time
        # (tiny layers at launch-bound batches: usf_coupling_tiny.hip does the same, and the backward chain in one launch)
        m["tiny"] = tiny
        if self.train and (tiny or (e.save_fused_hidden(cp, B) and op.u.coupling.split_in)):
            for j, hb in enumerate(e._hidden_bufs(ws, i, len(cp["hidden"]), B, self.device)):
                op.u.coupling.hidden_out[j] = hb.data_ptr()
            op.u.coupling.ld_hidden_out = e.hmax
            m["hidden_saved_fused"] = True
        if vctx:
            # a vector context: the launch becomes usf_coupling_additive_vctx_f32 -- a prefix op carries its arguments
            f = cp["fused"]
            self.ops.append(_ext.coupling_vctx_prefix(ws["ctx4"], ws["ctx4"].shape[1], e.ctx_dim, f["W_ctx_t"],
                                                      f["W_ctx_t"].shape[1], f["b_ctx"]))
            m["op"] = len(self.ops)
        self.ops.append(op)
        return True

    def _coupling_unfused(self, m: dict, cp: dict, zptr: int, sign: float) -> None:
        """the conditioner MLP as short linear launches through a pair of hidden buffers; the last one adds into z"""
        e, pk, ws, ops, B = self.eng, self.pk, self.ws, self.ops, self.B
        un = e._unfused_pack(pk, cp)
        # training: every hidden layer of every coupling keeps a buffer of its own -- the backward pass reads the activations
        # from there instead of running the conditioner a second time, at no cost to the forward
        # (USFLOWS_AMD_SAVE_HIDDEN=0: only up to GRAD_JOB_MAX_ROWS rows, where the step is bound by the number of its launches)
        save_h = self.train and B > 0 and (B <= _ext.GRAD_JOB_MAX_ROWS or config.save_hidden)
        m["hidden_saved"] = save_h
        n = len(un["layers"])
        hbufs = e._hidden_bufs(ws, m["step"], n, B, self.device) if save_h else [ws[("H1", "H2")[j % 2]] for j in range(n)]
        src_ptr, src_ld, src_K = zptr + 4 * cp["pass_off"], e.LD, cp["pass_n"]
        for j, (W, b) in enumerate(un["layers"]):
            hb = hbufs[j]
            kw = {}
            if j == 0 and m["use_ctx"]:
                # P = ctx . Wc^T + bc as a K = Cp GEMM (the context in columns [0, C) of a zero-padded [B, Cp] operand);
                # added to (acc + b_in) before the activation, as networks.py:741-745 does
                Cp = ws["ctx4"].shape[1]
                ops.append(linear_op(A=ws["ctx4"].data_ptr(), lda=Cp, W=un["W_ctx4"].data_ptr(), ldw=Cp,
                                     bias=un["b_ctx"].data_ptr(), C=ws["P"].data_ptr(), ldc=e.hmax,
                                     M=B, N=cp["hidden"][0], K=Cp, res_sign=1.0, slope=0.0, act=_ext.ACT_NONE))
                kw = dict(addend=ws["P"].data_ptr(), ldadd=e.hmax)
            kw.update(e._split_kw(pk, W, src_K))
            ops.append(linear_op(A=src_ptr, lda=src_ld, W=W.data_ptr(), ldw=W.shape[1], bias=b.data_ptr(),
                                 C=hb.data_ptr(), ldc=e.hmax, M=B, N=W.shape[0], K=src_K, res_sign=1.0,
                                 slope=cp["slope"], act=cp["act"], **kw))
            src_ptr, src_ld, src_K = hb.data_ptr(), e.hmax, W.shape[0]
        tptr = zptr + 4 * cp["tr_off"]
        ops.append(linear_op(A=src_ptr, lda=src_ld, W=un["W_out"].data_ptr(), ldw=un["W_out"].shape[1],
                             bias=un["b_out"].data_ptr(), residual=tptr, ldr=e.LD, C=tptr, ldc=e.LD,
                             M=B, N=cp["tr_n"], K=src_K, res_sign=sign, slope=0.0, act=_ext.ACT_NONE,
                             **e._split_kw(pk, un["W_out"], src_K)))

    def _coupling_general(self, cp: dict, zptr: int, sign: float) -> None:
        """the vector ConvNet conditioner with GatedMLP / LayerNormVector blocks (networks.py:206-245, 287-308) as a chain
        of linear launches and one row pass per block (usf_gated_norm_rows_f32: gate, layer norm and the activation in
        front of the next Linear in one kernel), then the masked residual in the last Linear's epilogue"""
        e, pk, ws, ops, B = self.eng, self.pk, self.ws, self.ops, self.B
        un = e._unfused_pack(pk, cp)
        hm = e.hmax

        def buf(name, width=hm):
            key = f"G_{name}"
            if key not in ws:
                ws[key] = torch.zeros(B, width, dtype=torch.float32, device=self.device)
            return ws[key]

        def linear(Wb, src, src_ld, dst, dst_ld, act=False, **extra):
            W, b = Wb
            K = W.shape[1]
            ops.append(linear_op(A=src, lda=src_ld, W=W.data_ptr(), ldw=K, bias=b.data_ptr(), C=dst, ldc=dst_ld, M=B,
                                 N=W.shape[0], K=K, res_sign=extra.pop("res_sign", 1.0), slope=cp["slope"] if act else 0.0,
                                 act=cp["act"] if act else _ext.ACT_NONE, **extra, **e._split_kw(pk, W, K)))

        def rows(*args, **kw):
            ops.append(gated_norm_op(B, cp, *args, **kw))

        hcur, hnext, A, T, S, VG = buf("H1"), buf("H2"), buf("A"), buf("T"), buf("S"), buf("VG", 2 * hm)
        linear(un["first"], zptr + 4 * cp["pass_off"], e.LD, hcur.data_ptr(), hm)
        rows(hcur, cp["raw"]["h"][0], None, A)          # a = f(h): the activation in front of block 0's Linear
        nb = len(un["blocks"])
        for j, blk in enumerate(un["blocks"]):
            wo = blk["w_out"]
            nxt_act = A if j + 1 < nb else None          # the final Linear has no activation in front of it
            if "lin" in blk:
                linear(blk["lin"], A.data_ptr(), hm, T.data_ptr(), hm)
                rows(T, wo, hnext, nxt_act, ln=blk.get("ln"), eps=blk["eps"])
            else:
                linear(blk["l1"], A.data_ptr(), hm, T.data_ptr(), hm, act=True)
                linear(blk["l2"], T.data_ptr(), hm, VG.data_ptr(), 2 * hm)
                skip = hcur
                if "proj" in blk:
                    linear(blk["proj"], hcur.data_ptr(), hm, S.data_ptr(), hm)
                    skip = S
                rows(skip, wo, hnext, nxt_act, vg=VG, gate_off=_round_up(wo, 4), ln=blk.get("ln"), eps=blk["eps"])
            hcur, hnext = hnext, hcur
        tptr = zptr + 4 * cp["tr_off"]
        linear((un["W_out"], un["b_out"]), hcur.data_ptr(), hm, tptr, e.LD, residual=tptr, ldr=e.LD, res_sign=sign)

    def result(self) -> dict:
        """the plan, with the layout fix-up behind the last op where the activations are not yet where ``final`` wants them"""
        e, ops, cur = self.eng, self.ops, self.cur
        final_gather = None
        if self.final == "user" and cur[0] != "user_out":
            final_gather = (cur, "user_out")
        elif self.final == "nat" and cur[1] != "nat":
            e._nat2(self.ws, self.B, self.device)
            final_gather = (cur, "nat2")
            cur = ("nat2", "nat", e.LDn)
        arr = (_ext.Op * max(len(ops), 1))(*ops)
        return dict(arr=arr, n=len(ops), patch_in=[(i_, "linear", "A") for i_ in self.patch_in],
                    patch_out=[(i_, "linear", "C") for i_ in self.patch_out], side=self.side,
                    final_gather=final_gather, out_buf=cur, ws=self.ws, pk=self.pk, meta=self.meta)
