"""The parameter-sized fp64 end of the flat flows' backward (map: training.py): the gradients the layer loops left in the
natural-layout stacks -> the LU factors' / Householder vectors' / ScaleTransform's gradients in the arena.

Plain functions of the parameter pack ``pk``, the gradient ``arena``, the ``stacks``, the recorded uses ``aff`` and the row maps
``lu`` (``lu_slots``); nothing here knows about plans' launches, workspaces or the layer loops."""
from __future__ import annotations

from typing import Dict, Optional

import torch

from . import _ext
from . import transforms as T


def grad_slot(arena, p: torch.Tensor) -> Optional[torch.Tensor]:
    """the parameter's view in the gradient arena (zeroed at the start of every backward)"""
    if not p.requires_grad:
        return None
    arena["touched"].add(id(p))
    return arena["views"].get(id(p))


def lu_slots(pk, meta) -> dict:
    """slot: id(affine block) -> row of the batched gradient stacks, when the batched chain rule applies (else None): every
    affine block is one LU factor -- bare, Sequential([LU]) or Sequential([LU, Householder with one vector]) (the USFlow
    constructor's default) --, used once in its M^-1 form and at most once in its M form (affine_conjugation),
    all LU factors prepared in one chunk.  hh: row -> Householder module (or absent); blocks: the blocks in row order."""
    chunks = pk["affine_parts"]["__chunks__"]
    none = dict(slot=None, hh={}, blocks=[])
    if len(chunks) != 1:
        return none
    idx = {id(lu): j for j, lu in enumerate(chunks[0]["lus"])}
    slots, hhs, by_row, seen = {}, {}, {}, set()
    for m in meta:
        if m["kind"] != "affine":
            continue
        blk = m["blk"]
        leaf, hh = blk, None
        if isinstance(blk, T.SequentialAffineTransform):
            parts = list(blk.transforms)
            if len(parts) == 1:
                leaf = parts[0]
            elif (len(parts) == 2 and isinstance(parts[1], T.HouseholderTransform) and parts[1].nvs == 1):
                leaf, hh = parts
        use = (id(leaf), m["prim"])
        if not isinstance(leaf, T.LUTransform) or use in seen or (m["prim"] == "affine_fwd" and m["pre_scale"] is not None):
            return none
        seen.add(use)
        slots[id(blk)] = idx[id(leaf)]
        by_row[idx[id(leaf)]] = blk
        if hh is not None:
            hhs[idx[id(leaf)]] = hh
    if {u[0] for u in seen if u[1] == "affine_bwd"} != set(idx):
        return none
    return dict(slot=slots, hh=hhs, blocks=[by_row[r] for r in sorted(by_row)])


def affine_param_grads(pk, arena, aff, stacks, lu, coef, g_lp, gsum):
    """coef: id(affine module) -> its log-det's sign in log_prob = base(z) - ladj_total, ladj_total = sum_steps (+/-) ladj(step)
    (flows.py:236-245); gsum: the gradient at the log-det output (None: sum(g_lp))"""
    dev = g_lp.device
    D = stacks["G"].shape[-1]
    Gsum = g_lp.double().sum() if gsum is None else gsum.double().reshape(())
    if lu["slot"] is not None:
        return _lu_chain_rule_batched(pk, arena, aff, stacks, lu, Gsum, coef)
    lu_acc: Dict[int, dict] = {}         # id(LUTransform) -> dict(dMinv, dM, db, c) fp64
    for rec in aff.values():
        blk = rec["blk"]
        prep = pk["affine"][id(blk)]
        dMinv = dM = None
        db = torch.zeros(D, dtype=torch.float64, device=dev)
        for u in rec["uses"]:
            G = u["G"].double()
            gs = u["gsum"].double()
            if u["which"] == "Minv":
                if u["pre_scale"] is not None:
                    G = _head_grad(u, prep["Minv"], G, gs, prep["b"], Gsum, arena)
                # y = (a - b) Minv^T:  dMinv = g^T a - gsum (x) b ,  db = -Minv^T gsum
                G = G - torch.outer(gs, prep["b"])
                dMinv = G if dMinv is None else dMinv + G
                db = db - prep["Minv"].t() @ gs
            else:
                # y = a M^T + b (InverseTransform.backward = block forward, transforms.py:370-376)
                dM = G if dM is None else dM + G
                db = db + gs
        _to_leaves(blk, prep, dMinv, dM, db, coef.get(id(blk), 0.0) * Gsum, lu_acc, arena, pk)
    _lu_param_grads(pk, lu_acc, arena, D)


def _head_grad(u, Minv, G, gs, b, Gsum, arena):
    """the first layer behind a ScaleTransform: a = x / s.  From G = g^T x returns g^T a = G diag(1/s) and writes
    ds_d = -(1/s_d^2) sum_n Minv[n,d] G[n,d] - Gsum / s_d   (transforms.py:116-144).  The planes pipeline's head packs
    a' = x / s - b, so there the weight gradient arrives as g^T a' and g^T x = (g^T a' + gsum (x) b) diag(s) comes first."""
    s64 = u["pre_scale"].scale.detach().double()
    if u.get("pre_sub_folded"):
        G = (G + torch.outer(gs, b)) * s64[None, :]
    gsc = grad_slot(arena, u["pre_scale"].scale)
    if gsc is not None:
        ds = -(Minv * G).sum(0) / (s64 * s64) - Gsum / s64
        gsc.copy_(ds.reshape(gsc.shape))
    return G / s64[None, :]


def _lu_chain_rule_batched(pk, arena, aff, stacks, lu, Gsum, coef):
    """One pass over [n, D, D] stacks for all affine blocks (block matrix M_t = M_lu H, H = the block's Householder
    factor or I; transforms.py:1457-1476):
        usage M_t^-1 (y = (a - b_t) M_t^-T):  dMinv_t = g^T a - gsum (x) b_t,   db_t = -M_t^-T gsum
        usage M_t    (y = a M_t^T + b_t)    :  dM_t = g^T a,                     db_t += gsum
        M_t^-1 = H^T M_lu^-1, M_t = M_lu H, b_t = b_lu H:
           dMinv_lu = H dMinv_t,  dM_lu = dM_t H^T,  db_lu = H db_t,
           dH = M_lu^-1 dMinv_t^T + M_lu^T dM_t + b_lu (x) db_t
        M_lu^-1 = U^-1 L^-1, M_lu = L U:
           dU = -triu(U^-T (dMinv_lu M_lu^-T)) + triu(L^T dM_lu) + c diag(1/U_jj)
           dL = -tril((M_lu^-T dMinv_lu) L^-T, -1) + tril(dM_lu U^T, -1)
        H = w_0 (I - 2 v v^T / v.v),  A = w_0^T dH:   dv = -2 (A + A^T) v / s + 4 (v^T A v) v / s^2,  s = v.v
    everything batched on the f64 MFMA (usf_gemm_f64) / batched torch ops."""
    ch = pk["affine_parts"]["__chunks__"][0]
    out = ch["out"]
    n, D = len(ch["lus"]), stacks["G"].shape[-1]
    DD = D * D
    dev = out["Minv"].device
    bat = dict(batch=n, M=D, N=D, K=D, lda=D, ldb=D, ldc=D, strideC=DD)
    f64 = lambda: torch.zeros(n, D, D, dtype=torch.float64, device=dev)
    Minv_lu, b_lu = out["Minv"], ch["b"]
    hh, blocks = lu["hh"], lu["blocks"]
    has_hh = bool(hh)
    if has_hh:
        # block-level matrices M_t^-1 / b_t and H per row (H = I where the block has no Householder factor)
        eye = stacks.setdefault("eye", torch.eye(D, dtype=torch.float64, device=dev))
        H = torch.stack([pk["affine_parts"][id(hh[j])]["M"] if j in hh else eye for j in range(n)])
        Minv_t = torch.stack([pk["affine"][id(b_)]["Minv"] for b_ in blocks])
        b_t = torch.stack([pk["affine"][id(b_)]["b"] for b_ in blocks])
    else:
        H, Minv_t, b_t = None, Minv_lu, b_lu
    G = stacks["G"][:n].double()
    gs = stacks["gs"][:n].double()
    for rec in aff.values():
        for u in rec["uses"]:
            if u["pre_scale"] is not None:
                k = u["row"]
                G[k] = _head_grad(u, Minv_t[k], G[k], gs[k], b_t[k], Gsum, arena)
    dMinv_t = G - gs[:, :, None] * b_t[:, None, :]
    # db_t = -M_t^-T gsum, one row-vector product per block on the library's batched fp64 kernel (no BLAS call on the path)
    db_t = torch.empty(n, D, dtype=torch.float64, device=dev)
    _ext.gemm_f64(gs.contiguous(), Minv_t.contiguous(), db_t, batch=n, M=1, N=D, K=D, lda=D, ldb=D, ldc=D, strideA=D, strideB=DD,
                  strideC=D, alpha=-1.0)
    dM_t = None
    if "GM" in stacks:
        dM_t = stacks["GM"][:n].double()
        db_t = db_t + stacks["gsM"][:n].double()
    if has_hh:
        dMinv_lu, dH = stacks.setdefault("dMinv_lu", f64()), stacks.setdefault("dH", f64())
        _ext.gemm_f64(H, dMinv_t, dMinv_lu, strideA=DD, strideB=DD, **bat)                    # H dMinv_t
        _ext.gemm_f64(Minv_lu, dMinv_t, dH, transB=True, strideA=DD, strideB=DD, **bat)       # M_lu^-1 dMinv_t^T
        db_lu = torch.bmm(H, db_t.unsqueeze(2)).squeeze(2)
        dH += b_lu[:, :, None] * db_t[:, None, :]
        dM_lu = None
        if dM_t is not None:
            dM_lu = stacks.setdefault("dM_lu", f64())
            _ext.gemm_f64(dM_t, H, dM_lu, transB=True, strideA=DD, strideB=DD, **bat)         # dM_t H^T
            _ext.gemm_f64(out["M"], dM_t, dH, transA=True, strideA=DD, strideB=DD, beta=1.0, **bat)   # + M_lu^T dM_t
        _householder_grads(dH, stacks, hh, arena, dev)
    else:
        dMinv_lu, dM_lu, db_lu = dMinv_t, dM_t, db_t
    # ---- LU factors
    tmp = stacks.get("T")
    if tmp is None:      # zero-filled once: tiles the masked products never write must stay finite for triu / tril
        tmp = stacks["T"] = torch.zeros(3, n, D, D, dtype=torch.float64, device=dev)
    T1, dU, dL = tmp[0], tmp[1], tmp[2]
    tinv = out["tri_inv"]                                   # [2n, D, D]: L^-1 at even, (U^-1)^T at odd rows
    # only one triangle of each result survives (triu / tril below) and the inverses are triangular: the tile masks
    # and k-range hints of usf_gemm_f64 cut the four products to ~3/8 of their dense cost
    _ext.gemm_f64(dMinv_lu, Minv_lu, T1, transB=True, strideA=DD, strideB=DD, tri=8, **bat)   # triu(G M^-T)
    _ext.gemm_f64(tinv, T1, dU, alpha=-1.0, strideA=2 * DD, strideB=DD, a_off=DD, tri=8 + 3, **bat)   # -U^-T (.)
    _ext.gemm_f64(Minv_lu, dMinv_lu, T1, transA=True, strideA=DD, strideB=DD, tri=16, **bat)  # tril(M^-T G)
    _ext.gemm_f64(T1, tinv, dL, transB=True, alpha=-1.0, strideA=DD, strideB=2 * DD, tri=16 + 4, **bat)  # -(.) L^-T
    if "coef" not in stacks:        # built once: a host-to-device copy here would drain the stream every step
        stacks["coef"] = torch.tensor([coef.get(id(b_), 0.0) for b_ in blocks], dtype=torch.float64, device=dev)
    c = stacks["coef"] * Gsum
    TL = TU = None
    if dM_lu is not None:
        # the M = L U usages:  dL += tril(G U^T, -1),  dU += triu(L^T G)
        tri = out["tri"]                                    # [2n, D, D]: L at even, U^T at odd rows
        TL, TU = tmp[0], stacks.setdefault("T2", f64())
        _ext.gemm_f64(dM_lu, tri, TL, strideA=DD, strideB=2 * DD, b_off=DD, tri=16, **bat)    # tril(G U^T)
        _ext.gemm_f64(tri, dM_lu, TU, transA=True, strideA=2 * DD, strideB=DD, tri=8, **bat)  # triu(L^T G)
    # tril(dL + TL, -1), triu(dU + TU) + diag(c / U_jj) (transforms.py:1303-1320) and the converting copies into the fp32
    # gradient arena: one pass (usf_lu_grad_finish_f64) instead of eight over [n, D, D] tensors
    base, _n = arena["lu_views"][0]
    flat = arena["flat"]
    _ext.lu_grad_finish(dL, dU, TL, TU, c.contiguous(), out["tri"], n, D, flat[base: base + n * DD],
                        flat[base + n * DD: base + 2 * n * DD])
    flat[base + 2 * n * DD: base + 2 * n * DD + n * D].view(n, D).copy_(db_lu)
    for lu_ in ch["lus"]:
        for name in ("L_raw", "U_raw", "bias_vector"):
            if getattr(lu_, name).requires_grad:
                arena["touched"].add(id(getattr(lu_, name)))


def _householder_grads(dH, stacks, hh, arena, dev):
    """dLoss/dv of H = w_0 (I - 2 v v^T / v.v) for the rows that have a Householder factor (one vector each)"""
    rows = sorted(hh)
    hhs = [hh[j] for j in rows]
    if "w0T" not in stacks:     # w_0 is a fixed permutation (requires_grad = False, transforms.py:789)
        stacks["w0T"] = torch.stack([h.w_0.detach().double().t() for h in hhs]).contiguous()
        stacks["hh_rows"] = torch.tensor(rows, dtype=torch.long, device=dev)
    A = torch.bmm(stacks["w0T"], dH[stacks["hh_rows"]])                          # w_0^T dH
    v = torch.stack([h.vk_householder.detach()[0].double() for h in hhs])        # [m, D]
    s_ = (v * v).sum(1, keepdim=True)
    Av = torch.bmm(A, v.unsqueeze(2)).squeeze(2)
    ATv = torch.bmm(A.transpose(1, 2), v.unsqueeze(2)).squeeze(2)
    vAv = (v * Av).sum(1, keepdim=True)
    dv = -2.0 * (Av + ATv) / s_ + 4.0 * vAv * v / (s_ * s_)
    for i, h in enumerate(hhs):
        g = grad_slot(arena, h.vk_householder)
        if g is not None:
            g.copy_(dv[i].reshape(g.shape))


def _lu_acc(lu_acc, lu):
    return lu_acc.setdefault(id(lu), dict(lu=lu, dMinv=None, dM=None, db=None, c=0.0))


def _to_leaves(blk, prep, dMinv, dM, db, ladj_coef, lu_acc, arena, pk):
    """gradients w.r.t. a block's (M^-1, M, bias) -> its LU factors' accumulators / Householder parameters"""
    if isinstance(blk, T.SequentialAffineTransform) and len(blk.transforms) == 1:
        blk = blk.transforms[0]              # eye @ M_1 == M_1: the same matrices
    if isinstance(blk, T.LUTransform):
        a = _lu_acc(lu_acc, blk)
        for k_, v in (("dMinv", dMinv), ("dM", dM), ("db", db)):
            if v is not None:
                a[k_] = v if a[k_] is None else a[k_] + v
        a["c"] = a["c"] + ladj_coef
        return
    # general composition: small torch graph over the prepared fp64 matrices of the parts
    parts = list(blk.transforms) if isinstance(blk, T.SequentialAffineTransform) else [blk]
    with torch.enable_grad():
        leaves, mats = [], []
        for t in parts:
            if isinstance(t, T.LUTransform):
                pr = pk["affine_parts"][id(t)]
                Mi = pr["Minv"].detach().clone().requires_grad_(True)
                Mm = pr["M"].detach().clone().requires_grad_(True)
                bb = pr["b"].detach().clone().requires_grad_(True)
                leaves.append(("lu", t, Mi, Mm, bb))
                mats.append((Mm, Mi, bb))
            elif isinstance(t, T.HouseholderTransform):
                Hw = t._construct_householder_permutation().double()        # differentiable w.r.t. vk
                leaves.append(("hh", t, Hw))
                mats.append((Hw, Hw.t(), torch.zeros(t.dim, dtype=torch.float64, device=Hw.device)))
            else:
                raise RuntimeError(f"usflows_amd internal: affine part {type(t).__name__} "
                                   "(validated in TrainPath._check_plan)")
        M, Minv, b = mats[0]
        for m_, mi_, b_ in mats[1:]:                     # transforms.py:1457-1476
            M = M @ m_
            b = b @ m_ + b_
            Minv = mi_ @ Minv
        proxy = (b * db).sum()
        if dMinv is not None:
            proxy = proxy + (Minv * dMinv).sum()
        if dM is not None:
            proxy = proxy + (M * dM).sum()
        wanted, owners = [], []
        for lf in leaves:
            if lf[0] == "lu":
                wanted += [lf[2], lf[3], lf[4]]
                owners += [(lf[1], "dMinv"), (lf[1], "dM"), (lf[1], "db")]
            else:
                for p in lf[1].parameters():
                    if p.requires_grad:
                        wanted.append(p)
                        owners.append((p, "param"))
        got = torch.autograd.grad(proxy, wanted, allow_unused=True)
    for (owner, kind), g in zip(owners, got):
        if kind == "param":
            if g is not None:
                slot = grad_slot(arena, owner)
                slot.add_(g.to(slot.dtype))
            continue
        a = _lu_acc(lu_acc, owner)
        if g is not None:
            a[kind] = g if a[kind] is None else a[kind] + g
    for a in [_lu_acc(lu_acc, lf[1]) for lf in leaves if lf[0] == "lu"]:      # the block's log-det is the sum of its LU parts'
        a["c"] = a["c"] + ladj_coef


def _lu_param_grads(pk, lu_acc, arena, D):
    """batched over all LU blocks: (dMinv, dM, db) -> (L_raw, U_raw, bias_vector).grad on the f64 MFMA"""
    if not lu_acc:
        return
    accs = list(lu_acc.values())
    n = len(accs)
    dev = pk["affine_parts"][id(accs[0]["lu"])]["Minv"].device
    DD = D * D
    stack = lambda key: torch.stack([pk["affine_parts"][id(a["lu"])][key] for a in accs]).contiguous()
    zeros = lambda: torch.zeros(D, D, dtype=torch.float64, device=dev)
    dL, dU = (torch.zeros(n, D, D, dtype=torch.float64, device=dev) for _ in range(2))
    bat = dict(batch=n, strideA=DD, strideB=DD, strideC=DD, M=D, N=D, K=D, lda=D, ldb=D, ldc=D)
    if any(a["dMinv"] is not None for a in accs):
        G = torch.stack([a["dMinv"] if a["dMinv"] is not None else zeros() for a in accs]).contiguous()
        Minv, Linv, UinvT = stack("Minv"), stack("Linv"), stack("Uinv_t")
        T1, T2 = torch.empty_like(G), torch.empty_like(G)
        _ext.gemm_f64(G, Minv, T1, transB=True, **bat)                       # G Minv^T
        _ext.gemm_f64(UinvT, T1, dU, alpha=-1.0, **bat)                      # -U^-T (G Minv^T)
        _ext.gemm_f64(Minv, G, T2, transA=True, **bat)                       # Minv^T G
        _ext.gemm_f64(T2, Linv, dL, transB=True, alpha=-1.0, **bat)          # -(Minv^T G) L^-T
    if any(a["dM"] is not None for a in accs):
        G = torch.stack([a["dM"] if a["dM"] is not None else zeros() for a in accs]).contiguous()
        L, Ut = stack("L"), stack("Ut")
        _ext.gemm_f64(G, Ut, dL, beta=1.0, **bat)                            # + G U^T
        _ext.gemm_f64(L, G, dU, transA=True, beta=1.0, **bat)                # + L^T G
    for i, a in enumerate(accs):
        lu = a["lu"]
        gU = grad_slot(arena, lu.U_raw)
        if gU is not None:
            du = dU[i].triu()
            if a["c"] is not None and not (isinstance(a["c"], float) and a["c"] == 0.0):
                # d/dU_jj of c * sum_j log|U_jj|  (transforms.py:1303-1320)
                du = du + torch.diag(a["c"] / lu.U_raw.detach().double().diagonal())
            gU.add_(du.to(gU.dtype))
        gL = grad_slot(arena, lu.L_raw)
        if gL is not None:
            gL.add_(dL[i].tril(-1).to(gL.dtype))
        gb = grad_slot(arena, lu.bias_vector)
        if gb is not None and a["db"] is not None:
            gb.add_(a["db"].to(gb.dtype))
