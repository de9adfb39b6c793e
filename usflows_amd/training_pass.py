"""What the two layer loops of the flat flows' backward share (map: training.py): the state of ONE backward pass (``Pass``), the
opening of a pass, the base density's gradients, an affine layer's way into the chain rule's stacks, and the parameter gradients
of one Linear layer (``linear_grads``) with the scatter helpers under it."""
from __future__ import annotations

from typing import Dict, Optional

import torch

from . import _ext
from .config import config
from .training_chain import affine_param_grads, grad_slot, lu_slots


def inverse_index(idx: torch.Tensor, D: int, device) -> torch.Tensor:
    """layout index (column -> feature, -1 = padding) -> int32 [D]: feature -> column"""
    inv = torch.full((D,), -1, dtype=torch.int32)
    for c, f in enumerate(idx.tolist()):
        if f >= 0:
            inv[f] = c
    return inv.to(device)


def ws_buf(ws, name, rows, cols, dtype=torch.float32):
    t = ws.get(name)
    if t is None or t.shape[0] != rows or t.shape[1] < cols:
        t = torch.zeros(rows, cols, dtype=dtype, device=ws["zA"].device)
        ws[name] = t
    return t


class Pass:
    """One backward pass over one plan while its launches are recorded: everything a layer function may rely on is a field of
    this object, made in ``TrainPath.backward`` and handed to the layer functions.  (The path itself keeps only what outlives a
    pass: ``_cur``, the input gradient's location and the caches keyed by layout / device -- ``path._inv``.)"""

    def __init__(self, path, plan, arena, want_dx: bool):
        eng = path.eng
        self.path, self.eng, self.flow, self.plan, self.arena = path, eng, path.flow, plan, arena
        self.ws, self.pk = plan["ws"], plan["pk"]
        self.dev, self.B, self.D = self.ws["zA"].device, self.ws["zA"].shape[0], eng.D
        self.want_dx = bool(want_dx)
        self.first_meta = plan["meta"][0] if plan["meta"] else None
        planes = bool(plan.get("planes_train"))
        # Small batches (the reference trains on 32 rows: tests/explib/mnist.yaml:34) on the fp32-row path: the ~260 weight / bias
        # gradients of a step wait and leave as ONE usf_grad_jobs_f32 launch behind the layer loop (training_rows.backward_body)
        self.defer = not planes and bool(path.defer_small_grads) and 0 < self.B <= _ext.GRAD_JOB_MAX_ROWS
        self.g_pending = False          # fp32 rows: the coupling layer before this one queued reads of the gradient's columns
        self.wmode = 1 if eng.gemm_mode == "bf16x3" else 0      # weight gradients on the same arithmetic as the GEMMs
        # planes: the reductions that end the weight gradients are queued (each with a workspace of its own) and leave as ONE
        # launch behind the layer loop, in front of the batched un-permute jobs that read their outputs (config.wreduce_jobs)
        self.wred = [] if planes and config.wreduce_jobs else None
        self.aff: Dict[int, dict] = {}  # id(block) -> natural-layout gradients of its usages
        # log-det: log_prob = base(z) - ladj_total, ladj_total = sum_steps (+/-) ladj(step)  (flows.py:236-245)
        self.coef: Dict[int, float] = {}
        for s in eng.steps:
            if s.kind == "affine":
                self.coef[id(s.module)] = self.coef.get(id(s.module), 0.0) + (1.0 if s.inverted else -1.0)
        self.lu = lu_slots(self.pk, plan["meta"])
        D, n_aff = self.D, max(sum(1 for m in plan["meta"] if m["kind"] == "affine"), 1)
        # the stacks the affine layers' natural-layout gradients land in: the batched chain rule's rows
        self.stacks = dict(G=torch.zeros(n_aff, D, D, dtype=torch.float32, device=self.dev),
                           gs=torch.zeros(n_aff, D, dtype=torch.float32, device=self.dev), next=0)
        if self.lu["slot"] is not None and any(m["kind"] == "affine" and m["prim"] == "affine_fwd" for m in plan["meta"]):
            # affine_conjugation: a block is also used in its M form (InverseTransform.backward): stacks of their own
            self.stacks["GM"] = torch.zeros_like(self.stacks["G"])
            self.stacks["gsM"] = torch.zeros_like(self.stacks["gs"])

    def need_dgrad(self, m) -> bool:
        """does the affine layer m hand a data gradient on?  (the first layer's is d log_prob / dx: only when asked for)"""
        return m is not self.first_meta or self.want_dx

    def buf(self, name, rows, cols, dtype=torch.float32):
        return ws_buf(self.ws, name, rows, cols, dtype)

    def inv_idx(self, layout: str) -> torch.Tensor:
        """layout index (column -> feature) inverted: feature -> column of that layout"""
        return self.cached((layout,), lambda: inverse_index(self.eng._idx(layout), self.D, self.dev))

    def cached(self, key: tuple, make) -> torch.Tensor:
        """a selector / constant that depends on the layouts and the device only: kept on the path, across passes"""
        inv = self.path._inv
        key = key + (str(self.dev),)
        if key not in inv:
            inv[key] = make().to(self.dev)
        return inv[key]

    def linear(self, A, a_off, lda, W, Cbuf, c_off, ldc, M, N, K, **kw):
        """one usf_linear_f32 launch (bf16x3 planes attached when the engine's mode wants them)"""
        planes = None
        if self.eng._wants_planes(W.shape[0], K) and W.shape[1] == K:
            planes = self.eng._split_planes(self.pk, W)
        _ext.linear(A, W, Cbuf, M=M, N=N, K=K, lda=lda, ldw=W.shape[1], ldc=ldc, a_off=a_off, c_off=c_off,
                    W_split=planes, **kw)

    # ---- gradient images -> the parameters' arena slots (queued scatter / un-permute jobs) ----
    def grad_slot(self, p) -> Optional[torch.Tensor]:
        return grad_slot(self.arena, p)

    def scatter_weight(self, p, img, rows_sel, n_rows, cols_sel, n_cols):
        g = self.grad_slot(p)
        if g is None:
            return
        if g.shape != (n_rows, n_cols):
            raise RuntimeError(f"usflows_amd internal: gradient image {n_rows}x{n_cols} vs parameter {tuple(g.shape)} "
                               "(shapes are validated in TrainPath._check_plan)")
        _ext.pack_weight(img, rows_sel, n_rows, cols_sel, n_cols, W=g, ldw=n_cols, ld_src=img.shape[1])

    def scatter_vec(self, p, vec_img, sel, n):
        g = self.grad_slot(p)
        if g is not None:
            _ext.pack_weight(vec_img, None, 1, sel, n, W=g, ldw=n, ld_src=vec_img.shape[1])

    def colsum_to(self, p, d, n, ld, sign):
        g = self.grad_slot(p)
        if g is not None:
            _ext.colsum(d, g, M=self.B, N=n, ldy=ld, alpha=sign)

    def chain_rule(self, glp):
        """the host op that ends both layer loops: the parameter-sized chain rule, redone on every replay"""
        _ext.host_op(lambda: affine_param_grads(self.pk, self.arena, self.aff, self.stacks, self.lu, self.coef, glp,
                                                self.path._cur["gsum"]))


def linear_grads(ps: Pass, Y, A, gW, weight, bias, sel, shape, sign, *, gb=None, fuse=False, blocked=None, **kw):
    """The parameter gradients of ONE Linear layer: the weight gradient sign * Y^T A into the image gW, scattered into
    ``weight``'s slot (sel = (row selector, column selector), shape = the parameter's), and the bias gradient = the column sums
    of sign * Y (bias None: the caller's business).
      gb given   the sums go into that image row and are scattered through the row selector
      gb None    they go straight into the bias's slot
      fuse       fp32 rows: the sums may ride in the weight-gradient pass (usf_wgrad_bias_f32) where the library serves the shape
      blocked    the planes path: Y and A are (planes, blocks per row, first block) and usf_wgrad_blocked_f32 carries the sums
                 into gb; the value is the reduce queue's entry for this call (training_planes.wq)
    kw: N, K (+ ldy, lda, y_off / a_off, mode on fp32 rows) exactly as the entry point takes them."""
    (rows_sel, cols_sel), (n_rows, n_cols) = sel, shape
    B, N, cs = ps.B, kw["N"], None          # cs: where the weight-gradient pass itself leaves the column sums
    if blocked is not None:
        cs = gb
        _ext.wgrad_blocked(*Y, *A, gW, M=B, ldg=gW.shape[1], alpha=sign, **(dict(colsum=gb, cs_alpha=sign) if gb is not None else {}),
                           **kw, **blocked)
    else:
        if (fuse and (gb is not None or N == n_rows) and not ps.defer and config.fused_bias
                and _ext.wgrad_bias_ok(B, N, kw["K"], kw["ldy"], kw["lda"], ps.wmode)):
            cs = gb if gb is not None else ps.grad_slot(bias)
        _ext.wgrad(Y, A, gW, M=B, ldg=gW.shape[1], alpha=sign, **kw, **(dict(colsum=cs, cs_alpha=sign) if cs is not None else {}))
    ps.scatter_weight(weight, gW, rows_sel, n_rows, cols_sel, n_cols)
    if bias is not None and gb is not None:
        if cs is None:
            _ext.colsum(Y, gb, M=B, N=N, ldy=kw["ldy"], alpha=sign, **({"y_off": kw["y_off"]} if "y_off" in kw else {}))
        ps.scatter_vec(bias, gb, rows_sel, n_rows)
    elif bias is not None and cs is None:
        ps.colsum_to(bias, Y, n_rows, kw["ldy"], sign)


# ---- the opening both layer loops share ------------------------------------------------------------------------------------
def open_pass(ps: Pass):
    """the arena zeroed and g_lp staged (one host op of the tape), the base density's tensors (scale: the radius of a radial
    base) and its parameter gradients.  Returns (glp, base, loc, scale)"""
    ws, path, B = ps.ws, ps.path, ps.B
    glp = ps.buf("g_lp", 1, B)[0, :B]
    _ext.host_op(lambda: (ps.arena["flat"].zero_(), glp.copy_(path._cur["g_lp"])))
    info = ps.flow._base_info(ps.dev)
    base, loc, scale = path._base_tensors(ws, info)
    zname, _, ldn = ps.plan["out_buf"]
    if info[0] == "radial":
        scale = ps.buf("radius", 1, B)[0, :B]                     # the forward left r = ||z - loc||_p here
    _base_param_grads(ps, ws[zname], ldn, glp, base, loc, scale)
    return glp, base, loc, scale


def latent_grad_rows(ps: Pass, glp, base, loc, scale, gA):
    """d sum(g_lp log_prob) / d latent as fp32 rows in gA (row stride of the latent buffer) and, for a radial base, d loc
    from the same rows"""
    zname, _, ldn = ps.plan["out_buf"]
    _ext.base_logprob_grad(ps.ws[zname], ldn, glp, ps.B, ps.D, base, loc, scale, gA, ldn)
    if ps.flow._base_info(gA.device)[0] == "radial":
        g_loc = ps.grad_slot(ps.flow.base_distribution.loc)
        if g_loc is not None:                                     # r depends on z - loc: d/dloc = -sum_m d/dz
            _ext.colsum(gA, g_loc, M=ps.B, N=ps.D, ldy=ldn, alpha=-1.0)


def _base_param_grads(ps: Pass, z, ldz, glp, base, loc, scale):
    """a trainable Laplace / Normal base: d/dloc, d/dscale_unconstrained of sum_m g_lp[m] log_prob[m] -- one pass over the
    latent (usf_base_param_grad_f32), then the softplus chain rule / the reduction of broadcast parameters on [D] tensors"""
    if not ps.path.base_extra_params():
        return
    bm = ps.path._locscale_base()
    D = ps.D
    tmp = ps.buf("base_pg", 2, D)
    _ext.base_param_grad(z, ldz, glp, ps.B, D, base, loc, scale, tmp)

    def finish():
        def to_shape(v, p):
            return v.reshape(p.shape) if p.numel() == D and p.dim() == 1 else v.sum().reshape(p.shape)
        g = ps.grad_slot(bm.loc)
        if g is not None:
            g.copy_(to_shape(tmp[0, :D], bm.loc))
        g = ps.grad_slot(bm.scale_unconstrained)
        if g is not None:
            raw = bm.scale_unconstrained.detach()
            g.copy_(to_shape(tmp[1, :D] * torch.sigmoid(raw).expand(D), bm.scale_unconstrained))
    _ext.host_op(finish)


def affine_grad_to_stack(ps: Pass, m, Gp, gs):
    """the tail of an affine layer's parameter gradients, on either path: the weight-gradient image Gp and the bias sums gs
    go back to the natural layout, into the block's row of the stacks (two queued un-permute jobs), and the use is recorded
    for the chain rule (training_chain.affine_param_grads)"""
    D, stacks, slot = ps.D, ps.stacks, ps.lu["slot"]
    blk = m["blk"]
    which = "Minv" if m["prim"] == "affine_bwd" else "M"
    k = slot[id(blk)] if slot is not None else stacks["next"]
    stacks["next"] += 1
    own = "M" if slot is not None and which == "M" else ""       # (batched chain rule: the M-form uses have stacks of their own)
    G_nat, gs_nat = stacks["G" + own][k], stacks["gs" + own][k]
    _ext.pack_weight(Gp, ps.inv_idx(m["out_layout"]), D, ps.inv_idx(m["in_layout"]), D, W=G_nat, ldw=D, ld_src=Gp.shape[1])
    _ext.pack_weight(gs, None, 1, ps.inv_idx(m["out_layout"]), D, W=gs_nat, ldw=D, ld_src=gs.shape[1])
    rec = ps.aff.setdefault(id(blk), dict(blk=blk, uses=[]))
    rec["uses"].append(dict(which=which, G=G_nat, gsum=gs_nat, pre_scale=m["pre_scale"], row=k,
                            pre_sub_folded=bool(m.get("pre_sub_folded"))))
