"""The flat flows' backward on fp32 rows (map: training.py): the layer loop, the affine layer, the dense and the general
(gated / layer-norm) coupling layer, and the weight images they read.  Every function takes the pass object first."""
from __future__ import annotations

import torch

from . import _ext
from .config import config
from .engine import _round_up, conditioner_layers
from .training_pass import (Pass, affine_grad_to_stack, inverse_index, latent_grad_rows, linear_grads, open_pass)


def backward_body(ps: Pass):
    """returns the input gradient's (buffer, row stride) when the pass was asked for it, else None"""
    eng, B = ps.eng, ps.B
    wid = max(eng.LD, eng.LDn)
    gA, gB = ps.buf("gA", B, wid), ps.buf("gB", B, wid)
    glp, base, loc, scale = open_pass(ps)
    latent_grad_rows(ps, glp, base, loc, scale, gA)
    g_cur, g_other, g_ld = gA, gB, ps.plan["out_buf"][2]
    prepare_images(ps)
    # gradient images -> parameter layout (scatter / un-permute): every layer has image buffers of its own, so all of these
    # copies wait in one batch and go out as one launch per size class behind the last layer.  Small batches (ps.defer): the
    # weight / bias gradient jobs wait as well, so their operands must outlive the layer loop: every layer gets gradient /
    # activation buffers of its own instead of the ping-pong pairs, and a coupling layer that would update, in place, columns a
    # queued job of the coupling layer before it still has to read flushes the queue first (ps.g_pending).
    with _ext.batch_jobs(ps.dev, defer_grads=ps.defer):
        for m in reversed(ps.plan["meta"]):
            if m["kind"] == "affine":
                g_cur, g_other, g_ld = affine_backward(ps, m, g_cur, g_other, g_ld)
                ps.g_pending = False
            else:
                coupling_backward(ps, m, g_cur, g_ld)
                ps.g_pending = ps.defer
    ps.chain_rule(glp)
    return (g_cur, g_ld) if ps.want_dx else None              # the gradient at the first layer's input (natural order)


def prepare_images(ps: Pass):
    """every weight image the backward reads (unfused conditioner layers, transposed images of the data-gradient
    GEMMs), built up front in two batched launches that join the pack's tape"""
    eng, pk, meta = ps.eng, ps.pk, ps.plan["meta"]
    with eng._pk_record(pk):
        with _ext.batch_jobs(ps.dev):
            for m in meta:
                if m["kind"] == "coupling":
                    eng._unfused_pack(pk, pk["coupling"][m["step"]])
        with _ext.batch_jobs(ps.dev):
            for m in meta:
                if m["kind"] == "coupling":
                    if fused_cbwd(ps, m):
                        eng._fused_pack_bwd(pk, pk["coupling"][m["step"]])      # the transposed set of the fused kernel
                        continue
                    un = eng._unfused_pack(pk, pk["coupling"][m["step"]])
                    if un.get("general"):
                        for W in [un["first"][0], un["W_out"]] + [e[k][0] for e in un["blocks"] for k in ("lin", "l1", "l2", "proj")
                                                                   if k in e]:
                            transposed(ps, W)
                        continue
                    for W, _b in un["layers"]:
                        transposed(ps, W)
                    transposed(ps, un["W_out"])
                elif ps.need_dgrad(m):
                    which = "Minv" if m["prim"] == "affine_bwd" else "M"
                    eng._mat(pk, m["blk"], which, m["out_layout"], m["in_layout"], transpose=True)


def fused_cbwd(ps: Pass, m) -> bool:
    """the data-gradient chain of this coupling layer's conditioner as ONE launch of the fused kernel (engine.
    coupling_backward_op): where the forward ran fused and left its hidden activations, unless USFLOWS_AMD_FUSED_CBWD=0"""
    # (queued gradient jobs read the d_h buffers after the layer loop: the tiny-layer form gives every layer buffers of its own)
    return bool(m.get("hidden_saved_fused")) and config.fused_cbwd and (bool(m.get("tiny")) or not ps.defer)


def transposed(ps: Pass, W: torch.Tensor) -> torch.Tensor:
    """[K, N4] image of W^T for a conditioner weight image W [N, K] (N padded to 4: it is the linear kernel's K),
    built from the raw parameter the image came from (no dependency on the image: both can sit in one batch)"""
    eng, pk = ps.eng, ps.pk
    key = ("T", W.data_ptr())
    if key not in pk["mats"]:
        N, K = W.shape
        N4 = _round_up(N, 4)
        Wt = torch.empty(K, N4, dtype=torch.float32, device=W.device)
        planes = None
        if eng._wants_planes(K, N4):
            planes = torch.empty(3, K, _round_up(N4, 32), dtype=torch.bfloat16, device=W.device)
        with eng._pk_record(pk):
            origin = pk["mats"].get(("imgsrc", W.data_ptr()))
            if origin is not None:
                src, out_sel, n_out, in_sel, n_in = origin           # W[o, c] = src[out_sel[o], in_sel[c]]
                rows = eng._sel(out_sel[:n_out].cpu(), N4, W.device) if N4 != n_out else out_sel
                _ext.pack_weight(src, in_sel, n_in, rows, N4, W=Wt, ldw=N4, planes=planes, transpose=True)
            else:
                _ext.flush_jobs()
                sel = eng._iarange(N, N4, W.device)
                _ext.pack_weight(W, None, K, sel, N4, W=Wt, ldw=N4, planes=planes, transpose=True)
        pk["mats"][key] = Wt
        if planes is not None:
            pk["mats"][("planes", Wt.data_ptr())] = planes
    return pk["mats"][key]


def _sel_inv(ps: Pass, idx: torch.Tensor) -> torch.Tensor:
    """segment selector (position -> feature) -> int32 [D]: feature -> position in the segment (-1: not in it)"""
    ps.path._inv[("keep", idx.data_ptr())] = idx                  # (the key below is its address: it must stay alive)
    return ps.cached(("selinv", idx.data_ptr()), lambda: inverse_index(idx, ps.D, ps.dev))


def _two_sel(ps: Pass, wo: int) -> torch.Tensor:
    """row selector of a GatedMLP's second Linear: parameter row i -> image row (value rows [0, wo) stay, gate rows
    [wo, 2 wo) sit at [wp, wp + wo), wp = wo rounded up to 4)"""
    return ps.cached(("twosel", wo), lambda: torch.cat([torch.arange(wo), torch.arange(wo) + _round_up(wo, 4)]).to(torch.int32))


# ---- affine layers --------------------------------------------------------------------------------
def affine_backward(ps: Pass, m, g_cur, g_other, g_ld):
    eng, ws, pk, B, dev = ps.eng, ps.ws, ps.pk, ps.B, ps.dev
    need_dgrad = ps.need_dgrad(m)
    blk = m["blk"]
    which = "Minv" if m["prim"] == "affine_bwd" else "M"
    n_out, n_in = (int(eng._idx_dev(m[k], dev).numel()) for k in ("out_layout", "in_layout"))
    # weight gradient in the image layout, then back to the natural [D, D] layout of the block's matrix
    wid = max(eng.LD, eng.LDn)
    Gp, gs = ps.buf(f"Gp{m['op']}", wid, wid), ps.buf(f"gs{m['op']}", 1, wid)   # own images per layer: their un-permute jobs run later
    # large batches: the data-gradient GEMM runs first and leaves the planes it makes of g; the weight gradient then
    # multiplies them with the planes the forward GEMM left of the layer input (no operand split in its loaders)
    from_planes = (need_dgrad and not ps.defer and ps.wmode == 1 and m.get("in_planes") is not None
                   and m["in_planes"] in ws and eng.wgrad_from_planes(B, n_out, n_in))
    if from_planes:
        gpl = ws.get("gpl")
        if gpl is None or gpl.shape[1] != -(-B // 32) * 32 or gpl.shape[2] < -(-n_out // 32) * 32:
            gpl = ws["gpl"] = _ext.row_planes(B, max(n_out, eng.LD, eng.LDn), dev)
        Wt = eng._mat(pk, blk, which, m["out_layout"], m["in_layout"], transpose=True)
        ps.linear(g_cur, 0, g_ld, Wt, g_other, 0, n_in, B, n_in, n_out, planes_out=gpl)
        cs_fused = (config.fused_bias                                                  # the bias gradient from the same pass
                    and bool(_ext.load().usf_wgrad_planes_colsum_ok(B, n_out, n_in)))
        _ext.wgrad_planes(gpl, ws[m["in_planes"]], Gp, M=B, N=n_out, K=n_in, ldg=Gp.shape[1], colsum=gs if cs_fused else None)
        if not cs_fused:
            _ext.colsum(g_cur, gs, M=B, N=n_out, ldy=g_ld)
    elif m["in_buf"] == "user_in":
        # the caller's tensor changes from call to call: issued through the wrapper on every replay
        path = ps.path
        _ext.host_op(lambda g=g_cur, ld=g_ld: _ext.wgrad(g, path._cur["x"], Gp, M=B, N=n_out, K=n_in, ldy=ld,
                                                        lda=path._cur["x"].shape[1], ldg=Gp.shape[1], mode=ps.wmode,
                                                        defer=False))
    else:
        _ext.wgrad(g_cur, ws[m["in_buf"]], Gp, M=B, N=n_out, K=n_in, ldy=g_ld, lda=m["in_ld"], ldg=Gp.shape[1], mode=ps.wmode)
    if not from_planes:
        _ext.colsum(g_cur, gs, M=B, N=n_out, ldy=g_ld)
    affine_grad_to_stack(ps, m, Gp, gs)
    if not need_dgrad:
        return g_cur, g_other, g_ld
    if not from_planes:
        Wt = eng._mat(pk, blk, which, m["out_layout"], m["in_layout"], transpose=True)
        # (deferred: g_cur waits for this layer's queued gradient jobs and is never written again)
        dst = ps.buf(f"gD{m['op']}", B, wid) if ps.defer else g_other
        ps.linear(g_cur, 0, g_ld, Wt, dst, 0, n_in, B, n_in, n_out)
        if ps.defer:
            return dst, g_other, n_in
    return g_other, g_cur, n_in


# ---- coupling layers ------------------------------------------------------------------------------
def coupling_backward_general(ps: Pass, m, g_cur, g_ld):
    """backward of a coupling layer whose conditioner is the vector ConvNet with GatedMLP / LayerNormVector blocks
    (reference networks.py:206-245, 287-308; forward: engine_flat._FlatPlan._coupling_general).  The conditioner runs once more from the
    layer's saved input with every intermediate kept (x_j, f(x_j), the hidden activations, [val, gate], the projected skip),
    then block by block backwards: usf_gated_norm_rows_bwd_f32 (layer norm + gate), usf_wgrad_f32 / usf_colsum_f32 for the
    parameters, usf_linear_f32 on the transposed images for the data gradients (the (Leaky)ReLU derivative in its epilogue:
    USF_ACT_GATE) -- what torch.autograd derives from the module under Flow.fit."""
    eng, ws, pk, B = ps.eng, ps.ws, ps.pk, ps.B
    cp = pk["coupling"][m["step"]]
    cond = eng.steps[m["step"]].module.conditioner
    un = eng._unfused_pack(pk, cp)
    raw, zbuf, sign = cp["raw"], ws[m["buf"]], m["sign"]
    LD, hm, act, slope = eng.LD, eng.hmax, cp["act"], cp["slope"]
    r4 = lambda n: _round_up(n, 4)                                 # noqa: E731
    own = f"_{m['step']}" if ps.defer else ""                      # (queued gradient jobs read these after the layer loop)
    buf = lambda tag, j, w=hm: ps.buf(f"GC{tag}{j}{own}", B, w)    # noqa: E731
    first_m, blocks_m, final_m = cond.block_view()
    nb, h0 = len(un["blocks"]), raw["h"][0]
    pass_n, pass_off, tr_n, tr_off = cp["pass_n"], cp["pass_off"], cp["tr_n"], cp["tr_off"]
    gate = lambda hbuf: dict(act=_ext.ACT_GATE, slope=slope, addend=hbuf, ldadd=hm) if act != _ext.ACT_NONE else {}   # noqa: E731
    # ---- 1. forward again, everything kept ----
    X = [buf("X", j) for j in range(nb + 1)]
    A = [buf("A", j) for j in range(nb)]
    Wf, bf = un["first"]
    ps.linear(zbuf, pass_off, LD, Wf, X[0], 0, hm, B, Wf.shape[0], pass_n, bias=bf)
    _ext.gated_norm_rows(X[0], M=B, C_cols=h0, c_pad=r4(h0), ld_skip=hm, out_act=A[0], ld_act=hm, act=act, slope=slope)
    Tb, VG, S = {}, {}, {}
    for j, e in enumerate(un["blocks"]):
        wi, wo = e["w_in"], e["w_out"]
        nxt = A[j + 1] if j + 1 < nb else None
        ln = e.get("ln")
        kw_ln = dict(gamma=ln[0], beta=ln[1], eps=e["eps"]) if ln is not None else {}
        kw_act = dict(out_act=nxt, ld_act=hm, act=act, slope=slope) if nxt is not None else {}
        Tb[j] = buf("T", j)
        if "lin" in e:
            W, b = e["lin"]
            ps.linear(A[j], 0, hm, W, Tb[j], 0, hm, B, W.shape[0], W.shape[1], bias=b)
            _ext.gated_norm_rows(Tb[j], M=B, C_cols=wo, c_pad=r4(wo), ld_skip=hm, out=X[j + 1], ld_out=hm, **kw_ln, **kw_act)
        else:
            W1, b1 = e["l1"]
            W2, b2 = e["l2"]
            ps.linear(A[j], 0, hm, W1, Tb[j], 0, hm, B, W1.shape[0], W1.shape[1], bias=b1, act=act, slope=slope)
            VG[j] = buf("VG", j, 2 * hm)
            ps.linear(Tb[j], 0, hm, W2, VG[j], 0, 2 * hm, B, W2.shape[0], W2.shape[1], bias=b2)
            skip = X[j]
            if "proj" in e:
                Wp, bp = e["proj"]
                S[j] = buf("S", j)
                ps.linear(X[j], 0, hm, Wp, S[j], 0, hm, B, Wp.shape[0], Wp.shape[1], bias=bp)
                skip = S[j]
            _ext.gated_norm_rows(skip, M=B, C_cols=wo, c_pad=r4(wo), ld_skip=hm, vg=VG[j], ld_vg=2 * hm, gate_off=r4(wo),
                                 out=X[j + 1], ld_out=hm, **kw_ln, **kw_act)
    # ---- 2. the output Linear: Y = the gradient at the transformed half, A = x_nb ----
    gimg = lambda tag: ps.buf(f"gWG{m['step']}_{tag}", max(2 * hm, LD), max(hm, LD))     # noqa: E731
    # one Linear layer's parameter gradients, Y [B, N] (row stride ldy) against A [B, K] (row stride hm)
    lin = lambda Y, A_, tag, W, mod, shape, ldy=hm, cols_sel=None: linear_grads(                     # noqa: E731
        ps, Y, A_, gimg(tag), mod.weight, mod.bias, (None, cols_sel), shape, sign,
        N=W.shape[0], K=W.shape[1], ldy=ldy, lda=hm, mode=ps.wmode)
    W_out = un["W_out"]
    w_last = un["blocks"][-1]["w_out"]
    tsel = _sel_inv(ps, raw["tr_idx"])
    linear_grads(ps, g_cur, X[nb], gimg("out"), final_m.weight, final_m.bias, (tsel, None), (eng.D, w_last), sign,
                 gb=ps.buf(f"gbG{m['step']}_out", 1, max(2 * hm, LD)), N=tr_n, K=W_out.shape[1], ldy=g_ld, lda=hm, y_off=tr_off,
                 mode=ps.wmode)
    DX = [buf("DX", j) for j in range(nb + 1)]
    Wt = transposed(ps, W_out)
    ps.linear(g_cur, tr_off, g_ld, Wt, DX[nb], 0, hm, B, Wt.shape[0], Wt.shape[1])
    # ---- 3. the blocks, last to first ----
    for j in range(nb - 1, -1, -1):
        e, bm = un["blocks"][j], blocks_m[j]
        wi, wo = e["w_in"], e["w_out"]
        ln = e.get("ln")
        gated = "lin" not in e
        skip = Tb[j] if not gated else (S[j] if "proj" in e else X[j])
        DR = buf("DR", j)
        DVG = buf("DVG", j, 2 * hm) if gated else None
        DYX = buf("DYX", j) if ln is not None else None
        _ext.gated_norm_rows_bwd(skip, DX[j + 1], DR, M=B, C_cols=wo, c_pad=r4(wo), ld_skip=hm, ld_dy=hm, ld_d_skip=hm,
                                 vg=VG.get(j), ld_vg=2 * hm, gate_off=r4(wo), d_vg=DVG, ld_d_vg=2 * hm,
                                 gamma=None if ln is None else ln[0], eps=e["eps"], dy_xh=DYX, ld_dy_xh=hm)
        if ln is not None:
            ps.colsum_to(bm["ln"].weight, DYX, wo, hm, sign)
            ps.colsum_to(bm["ln"].bias, DX[j + 1], wo, hm, sign)
        if not gated:
            W, _b = e["lin"]
            lin(DR, A[j], f"l{j}", W, bm["lin"], (wo, wi))
            Wt = transposed(ps, W)
            ps.linear(DR, 0, hm, Wt, DX[j], 0, hm, B, Wt.shape[0], Wt.shape[1], **gate(X[j]))
            continue
        W1, _b1 = e["l1"]
        W2, _b2 = e["l2"]
        # second Linear: Y = d[val, gate] (value rows [0, wp), gate rows [wp, 2 wp)), A = the hidden activations; its bias's two
        # halves are two column sums of their own
        linear_grads(ps, DVG, Tb[j], gimg(f"b{j}"), bm["l2"].weight, None, (_two_sel(ps, wo), None), (2 * wo, wo), sign,
                     N=W2.shape[0], K=W2.shape[1], ldy=2 * hm, lda=hm, mode=ps.wmode)
        g2 = ps.grad_slot(bm["l2"].bias)
        if g2 is not None:
            _ext.colsum(DVG, g2[:wo], M=B, N=wo, ldy=2 * hm, alpha=sign)
            _ext.colsum(DVG, g2[wo:], M=B, N=wo, ldy=2 * hm, y_off=r4(wo), alpha=sign)
        DT = buf("DT", j)
        Wt2 = transposed(ps, W2)
        ps.linear(DVG, 0, 2 * hm, Wt2, DT, 0, hm, B, Wt2.shape[0], Wt2.shape[1], **gate(Tb[j]))
        lin(DT, A[j], f"a{j}", W1, bm["l1"], (wo, wi))
        Wt1 = transposed(ps, W1)
        if "proj" in e:
            Wp, _bp = e["proj"]
            lin(DR, X[j], f"p{j}", Wp, bm["proj"], (wo, wi))
            # d x_j = f'(x_j) (dT W1) + dr Wp
            ps.linear(DT, 0, hm, Wt1, DX[j], 0, hm, B, Wt1.shape[0], Wt1.shape[1], **gate(X[j]))
            Wtp = transposed(ps, Wp)
            ps.linear(DR, 0, hm, Wtp, DX[j], 0, hm, B, Wtp.shape[0], Wtp.shape[1], residual=DX[j], ldr=hm)
        else:
            # d x_j = f'(x_j) (dT W1) + dr (the skip connection; USF_ACT_GATE takes no residual: one elementwise launch more)
            ps.linear(DT, 0, hm, Wt1, DX[j], 0, hm, B, Wt1.shape[0], Wt1.shape[1], **gate(X[j]))
            _ext.add_rows(DX[j], DR, ps.cached(("ones", hm), lambda: torch.ones(hm, dtype=torch.float32)))
    # ---- 4. the first Linear and the conditioning half of the gradient ----
    linear_grads(ps, DX[0], zbuf, gimg("in"), first_m.weight, first_m.bias, (None, _sel_inv(ps, raw["pass_idx"])), (h0, eng.D),
                 sign, N=Wf.shape[0], K=pass_n, ldy=hm, lda=LD, a_off=pass_off, mode=ps.wmode)
    if ps.g_pending:
        _ext.flush_jobs()          # the coupling layer before this one queued reads of columns this update rewrites
    Wtf = transposed(ps, Wf)
    ps.linear(DX[0], 0, hm, Wtf, g_cur, pass_off, g_ld, B, pass_n, Wtf.shape[1],
              residual=g_cur, r_off=pass_off, ldr=g_ld, res_sign=sign)


def coupling_backward(ps: Pass, m, g_cur, g_ld):
    eng, ws, pk, B = ps.eng, ps.ws, ps.pk, ps.B
    cp = pk["coupling"][m["step"]]
    if cp.get("general"):
        return coupling_backward_general(ps, m, g_cur, g_ld)
    cond = eng.steps[m["step"]].module.conditioner
    un = eng._unfused_pack(pk, cp)
    raw, zbuf, sign = cp["raw"], ws[m["buf"]], m["sign"]
    LD, hmax, act, slope = eng.LD, eng.hmax, cp["act"], cp["slope"]
    h, hp, nl = raw["h"], cp["hidden"], len(un["layers"])
    pass_n, pass_off, tr_n, tr_off = cp["pass_n"], cp["pass_off"], cp["tr_n"], cp["tr_off"]
    # 1. hidden activations again (the conditioning half of the saved buffer is what the forward saw)
    saved_fused = bool(m.get("hidden_saved_fused"))       # large batches: the fused forward kernel left them (engine_flat.py)
    saved = saved_fused or bool(m.get("hidden_saved"))    # ... or the unfused forward's GEMMs wrote them into the layer's own buffers
    own = f"_{m['step']}" if (ps.defer or saved) else ""            # deferred gradient jobs read these after the layer loop
    # (the layer's own buffers are the forward plan's -- engine_flat.py, `_hidden_bufs`; without them a shared set, recomputed)
    hbufs = eng._hidden_bufs(ws, m["step"], nl, B, zbuf.device) if own else [ps.buf(f"Hs{j}", B, hmax) for j in range(nl)]
    src, src_off, src_ld, src_K = zbuf, pass_off, LD, pass_n
    # (small batches: the forward plan left the hidden activations in exactly these buffers -- engine_flat.py, `hidden_saved`)
    for j, (W, b) in enumerate(un["layers"] if not saved else []):
        kw = {}
        if j == 0 and m["use_ctx"]:
            Cp = ws["ctx4"].shape[1]          # the context GEMM at K = Cp (context_dim padded to 4), as the forward plan's
            ps.linear(ws["ctx4"], 0, Cp, un["W_ctx4"], ws["P"], 0, hmax, B, hp[0], Cp, bias=un["b_ctx"])
            kw = dict(addend=ws["P"], ldadd=hmax)
        ps.linear(src, src_off, src_ld, W, hbufs[j], 0, hmax, B, W.shape[0], src_K, bias=b, act=act, slope=slope, **kw)
        src, src_off, src_ld, src_K = hbufs[j], 0, hmax, W.shape[0]
    first_l, ctx_l, hidden_l, last_l = conditioner_layers(cond)
    fused_bwd = fused_cbwd(ps, m)
    if fused_bwd:
        # ONE launch: g_P += s * MLP^T(g_T) with the (Leaky)ReLU backward from the saved activations; the gradients at the
        # hidden activations land in Dh{j} for the weight gradients below
        dh = [ps.buf(f"DhF{j}{own if ps.defer else ''}", B, hmax) for j in range(nl)]
        op = eng.coupling_backward_op(pk, cp, g_cur.data_ptr(), g_ld, B, sign, hbufs, dh,
                                      act=_ext.ACT_GATE if act != _ext.ACT_NONE else _ext.ACT_NONE)
        if ps.g_pending:
            _ext.flush_jobs()      # the coupling layer before this one queued reads of columns this launch rewrites
        _ext.coupling_op(op, raw["device"])
    # 2. output layer: d_out = gradient at the transformed half (unchanged by the layer: out_T = z_T + s MLP)
    W_out = un["W_out"]                                   # [tr_n, hp_last]
    gimg = lambda tag, cols=0: ps.buf(f"gW{m['step']}_{tag}", max(hmax, LD), max(hmax, LD, cols))      # noqa: E731
    # one Linear layer's parameter gradients, Y [B, N] (the gradient at its output) against A [B, K] (row stride lda); large
    # batches: the bias gradient rides in the weight-gradient pass (fuse)
    lin = lambda Y, A_, tag, mod, N, K, lda, shape, cols_sel=None, **kw: linear_grads(               # noqa: E731
        ps, Y, A_, gimg(tag), mod.weight, mod.bias, (None, cols_sel), shape, sign, fuse=True, N=N, K=K, ldy=hmax, lda=lda,
        mode=ps.wmode, **kw)
    tsel = _sel_inv(ps, raw["tr_idx"])
    linear_grads(ps, g_cur, hbufs[-1], gimg("out"), last_l.weight, last_l.bias, (tsel, None), (eng.D, h[-1]), sign,
                 gb=ps.buf(f"gb{m['step']}", 1, max(hmax, LD)), fuse=True, N=tr_n, K=hp[-1], ldy=g_ld, lda=hmax, y_off=tr_off,
                 mode=ps.wmode)
    # d_h = d_out W_out  (sign is applied where the result leaves the MLP)
    if ps.defer:                                              # d_bufs[j]: the gradient at hidden layer j's output
        d_bufs = [ps.buf(f"Dh{j}{own}", B, hmax) for j in range(nl)]
    else:
        pair = [ps.buf("Dh0", B, hmax), ps.buf("Dh1", B, hmax)]
        d_bufs = [pair[(nl - 1 - j) & 1] for j in range(nl)]
    if fused_bwd:
        d_bufs = dh
    d = d_bufs[nl - 1]
    # (the (Leaky)ReLU backward from the saved layer output rides in the GEMM's epilogue: USF_ACT_GATE)
    gate = lambda hbuf: dict(act=_ext.ACT_GATE, slope=slope, addend=hbuf, ldadd=hmax) if act != _ext.ACT_NONE else {}   # noqa: E731
    if not fused_bwd:
        Wt = transposed(ps, W_out)                        # [hp_last, tr_n4]
        ps.linear(g_cur, tr_off, g_ld, Wt, d, 0, hmax, B, hp[-1], Wt.shape[1], **gate(hbufs[-1]))
    # 3. hidden layers, last to first
    for j in range(nl - 1, 0, -1):
        W, _b = un["layers"][j]                           # [hp_j, hp_{j-1}]
        lin(d, hbufs[j - 1], f"h{j}", hidden_l[j - 1], hp[j], hp[j - 1], hmax, (h[j], h[j - 1]))
        if not fused_bwd:
            ps.linear(d, 0, hmax, transposed(ps, W), d_bufs[j - 1], 0, hmax, B, hp[j - 1], hp[j], **gate(hbufs[j - 1]))
        d = d_bufs[j - 1]
    # 4. input layer
    W_in, _b = un["layers"][0]                            # [hp0, pass_n]
    lin(d, zbuf, "in", first_l, hp[0], pass_n, LD, (h[0], eng.D), _sel_inv(ps, raw["pass_idx"]), a_off=pass_off)
    if ctx_l is not None and m["use_ctx"]:
        # d W_ctx [h0, C] = sign * d^T ctx over the padded context rows [B, Cp] (the padding columns hold zeros)
        # (an image of its own shape: Cp may be wider than every hidden layer and the rows, e.g. hidden [16] with C = 32)
        Cp = ws["ctx4"].shape[1]
        linear_grads(ps, d, ws["ctx4"], gimg("ctx", Cp), ctx_l.weight, ctx_l.bias, (None, None), (h[0], eng.ctx_dim), sign,
                     N=hp[0], K=Cp, ldy=hmax, lda=Cp)
    # conditioning half of the gradient: g_P += s * d W_in   (in place)
    if fused_bwd:
        return                     # (the fused launch above already updated the conditioning half)
    if ps.g_pending:
        _ext.flush_jobs()          # the coupling layer before this one queued reads of columns this update rewrites
    ps.linear(d, 0, hmax, transposed(ps, W_in), g_cur, pass_off, g_ld, B, pass_n, hp[0],
              residual=g_cur, r_off=pass_off, ldr=g_ld, res_sign=sign)
