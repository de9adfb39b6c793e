"""The flat flows' backward on the planes pipeline (map: training.py).

The forward ran as the inference pipeline does -- usf_pack_planes_f32, usf_gemm_planes_bf16x3, usf_coupling_planes --
with every affine output in a planes buffer of its own and the conditioners' hidden activations saved as planes
(engine._build_plan_planes(train=True)).  Backwards, layer by layer on a pair of gradient planes buffers:
  affine    usf_wgrad_blocked_f32 (gradient planes x saved input planes; the bias gradient from the same pass), then the
            data gradient = usf_gemm_planes_bf16x3 on the transposed weight planes
  coupling  ONE usf_coupling_planes launch in gate mode (the conditioner's transposed chain with leaky_relu_backward
            from the saved activations; it leaves the gradients at the pre-activations as planes), then the three
            weight gradients on usf_wgrad_blocked_f32
No fp32 row buffer and no operand split anywhere in the loop; the parameter-sized chain rule is training_chain's."""
from __future__ import annotations

import torch

from . import _ext
from .engine import conditioner_layers
from .training_pass import Pass, affine_grad_to_stack, latent_grad_rows, linear_grads, open_pass


def _planes_buf(ps: Pass, name, blocks):
    n = (-(-ps.B // 16)) * blocks * 3072
    t = ps.ws.get(name)
    if t is None or t.numel() < n:
        t = ps.ws[name] = torch.zeros(n, dtype=torch.uint8, device=ps.dev)
    return t


def _block_idx(ps: Pass, key, n, n_valid):
    """int32 [n]: column -> feature of a planes buffer that holds features 0 .. n_valid - 1 in their natural order"""
    return ps.cached(key, lambda: torch.cat([torch.arange(n_valid, dtype=torch.int32),
                                             torch.full((n - n_valid,), -1, dtype=torch.int32)]))


def backward_body(ps: Pass):
    """(no input gradient from here: the planes backward ends in planes of the first layer's operand)"""
    eng, ws, pk, B, D, dev, meta = ps.eng, ps.ws, ps.pk, ps.B, ps.D, ps.dev, ps.plan["meta"]
    nkb = eng.LDp // 32
    nkb_g = max(eng.LDp, eng.LDnp) // 32
    gA = ps.buf("gA", B, max(eng.LD, eng.LDn))
    glp, base, loc, scale = open_pass(ps)
    zname, _, ldn = ps.plan["out_buf"]
    radial = ps.flow._base_info(dev)[0] == "radial"
    gp = [_planes_buf(ps, "pgA", nkb_g), _planes_buf(ps, "pgB", nkb_g)]
    idx = _block_idx(ps, ("natp_g", nkb_g), 32 * nkb_g, D)
    if not radial and (16 * (D + 1) + 96 * nkb_g) * 4 <= 65536:      # (the rows kernel's LDS: 16 rows + the layout tables)
        # Laplace / Normal base: the gradient at the latent goes straight into the planes (one pass over z instead of
        # usf_base_logprob_grad_f32's fp32 rows + their repack)
        _ext.pack_planes(ws[zname], gp[0], M=B, nkb=nkb_g, idx=idx, ld=ldn, src_cols=D, grad=(base, glp, loc, scale))
    else:
        latent_grad_rows(ps, glp, base, loc, scale, gA)
        _ext.pack_planes(gA, gp[0], M=B, nkb=nkb_g, idx=idx, ld=ldn, src_cols=D)
    cur = 0
    with eng._pk_record(pk), _ext.batch_jobs(dev):      # every weight image of the backward, one batched launch
        for m in meta:
            if m["kind"] == "coupling":
                eng.planes_coupling_bwd(pk, m)
            elif ps.need_dgrad(m):
                eng.planes_dgrad_image(pk, m)
    if any(m["kind"] == "coupling" and m["use_ctx"] for m in meta):
        # the context as a one-block planes buffer (column 0 = ctx, the rest zero), packed once per step: the operand of every
        # context layer's weight gradient (usf_wgrad_blocked_f32 against the gradients at the first pre-activations)
        _ext.pack_planes(ws["ctx"], _planes_buf(ps, "pctx", 1), M=B, nkb=1, idx=_block_idx(ps, ("ctx_col",), 32, 1), ld=1)
    with _ext.batch_jobs(dev):
        for m in reversed(meta):
            if m["kind"] == "affine":
                cur = affine_backward(ps, m, gp, cur, nkb, nkb_g)
            else:
                coupling_backward(ps, m, gp[cur], nkb, nkb_g)
        if ps.wred:
            _ext.wgrad_reduce_flush(ps.wred, dev)
    ps.chain_rule(glp)


def wq(ps: Pass, tag, N, K) -> dict:
    """queue + a workspace of this call's own for usf_wgrad_blocked_plan_f32 (empty: the undeferred call)"""
    if ps.wred is None:
        return {}
    return dict(queue=ps.wred, ws=ps.buf(f"WGws{tag}", 1, _ext.wgrad_blocked_workspace(ps.B, N, K)))


def affine_backward(ps: Pass, m, gp, cur, nkb, nkb_g):
    eng, ws, B = ps.eng, ps.ws, ps.B
    n_out, n_in = m["N"], m["K"]
    wid = max(eng.LD, eng.LDn)
    Gp, gs = ps.buf(f"Gp{m['op']}", wid, wid), ps.buf(f"gs{m['op']}", 1, wid)
    _ext.wgrad_blocked(gp[cur], nkb_g, 0, ws[m["in_buf"]], nkb, 0, Gp, M=B, N=n_out, K=n_in, ldg=Gp.shape[1], colsum=gs,
                       **wq(ps, f"a{m['op']}", n_out, n_in))
    affine_grad_to_stack(ps, m, Gp, gs)
    if not ps.need_dgrad(m):
        return cur
    Wt = eng.planes_dgrad_image(ps.pk, m)
    nk = (eng.LDnp if m["out_layout"] == "natp" else eng.LDp) // 32
    _ext.gemm_planes(gp[cur], Wt, M=B, a_nkb=nkb_g, nk=nk, C_planes=gp[1 - cur], c_nkb=nkb_g, c_kb0=0, c_kbn=nkb)
    return 1 - cur


def _seg_sel(ps: Pass, m, which: str) -> torch.Tensor:
    """int32 [D]: feature -> position relative to the first block of the coupling's conditioning ('p') / transformed ('t')
    block range (-1: the feature is not in that set)"""
    def make():
        feat = m["feat_p"] if which == "p" else m["feat_t"]
        kb0 = m["kb_p0"] if which == "p" else m["kb_t0"]
        sel = torch.full((ps.D,), -1, dtype=torch.int32)
        for pos, f in enumerate(feat.tolist()):
            if f >= 0:
                sel[f] = pos - 32 * kb0
        return sel
    return ps.cached(("segsel", m["step"], which), make)


def coupling_backward(ps: Pass, m, g, nkb, nkb_g):
    eng, ws, pk, B = ps.eng, ps.ws, ps.pk, ps.B
    cp = pk["coupling"][m["step"]]
    cond = eng.steps[m["step"]].module.conditioner
    dev, h, sign = cp["raw"]["device"], list(cp["raw"]["h"]), m["sign"]
    nl = len(h)
    hs = [ws[n_] for n_ in m["hidden_planes"]]
    dh = [_planes_buf(ps, f"pD{j}", 8) for j in range(nl)]
    _ext.coupling_planes_op(eng.planes_coupling_bwd_op(pk, m, g, nkb_g, B, hs, dh), dev)
    first_l, ctx_l, hidden_l, last_l = conditioner_layers(cond)
    wmax = max(eng.LDp, 256)
    gvec = lambda tag: ps.buf(f"gb{m['step']}_{tag}", 1, wmax)          # noqa: E731
    # one Linear layer's parameter gradients: Y, A = (planes, blocks per row, first block), images of this layer's own
    lin = lambda Y, A, tag, q, mod, gb, sel, shape, N, K: linear_grads(                               # noqa: E731
        ps, Y, A, ps.buf(f"gW{m['step']}_{tag}", wmax, wmax), mod.weight, None if gb is None else mod.bias, sel, shape, sign,
        gb=gb, blocked=wq(ps, f"c{m['step']}{q}", N, K), N=N, K=K)
    # output layer: Y = the gradient at the transformed blocks (unchanged by the launch above), A = the last hidden activations
    n_t, n_p = m["n_t"], m["n_p"]                         # valid widths of the block ranges (engine_planes: _coupling_geometry)
    lin((g, nkb_g, m["kb_t0"]), (hs[nl - 1], 8, 0), "out", "o", last_l, gvec("out"), (_seg_sel(ps, m, "t"), None), (eng.D, h[-1]),
        n_t, 256)
    # hidden layers, last to first: Y = the gradient at layer j's pre-activation, A = layer j - 1's activations
    for j in range(nl - 1, 0, -1):
        lin((dh[j], 8, 0), (hs[j - 1], 8, 0), f"h{j}", f"h{j}", hidden_l[j - 1], gvec(f"h{j}"), (None, None), (h[j], h[j - 1]),
            h[j], 256)
    # input layer: A = the conditioning blocks of the layer's own z buffer (what the forward's conditioner saw)
    gb = gvec("in")
    lin((dh[0], 8, 0), (ws[m["buf"]], nkb, m["kb_p0"]), "in", "i", first_l, gb, (None, _seg_sel(ps, m, "p")), (h[0], eng.D),
        h[0], n_p)
    if ctx_l is not None and m["use_ctx"]:
        # the context layer (layers[1], context_dim 1 on this path) adds ctx * W_ctx + b_ctx to the first pre-activation: d b_ctx is the
        # column sum d b_in already holds, d W_ctx[h] = sign * sum_rows ctx[row] * d_h0[row, h] -- column 0 of the weight
        # gradient against the context planes.  (A context layer that sees no context gets no gradient, as under autograd.)
        ps.scatter_vec(ctx_l.bias, gb, None, h[0])
        lin((dh[0], 8, 0), (ws["pctx"], 1, 0), "ctx", "c", ctx_l, None, (None, None), (h[0], 1), h[0], 32)
