"""Cases, inputs, the fp64 reference, the checker and a numpy fp32 statement of the summation order of
usf_channel_affine_bwd_f32 (test_channel_affine_bwd_cpu.py, test_channel_affine_bwd_gpu.py).

A case is (B, C, P, form, cap): form names the operands ("plain": dx, dW, db; "presub": with pre_sub; "presub_nodx": pre_sub and
no dx; "nodb": no db; "+unaligned": x and dy start 4 bytes off a 16-byte boundary, which forces the scalar form where
P % 4 == 0); cap > 0 is the tuning aid channel_affine_bwd_blocks (the grid capped at so many blocks: several loop trips per
thread at a small size)."""
import numpy as np
import torch

TOL = 2e-6                 # of max|ref|: test_wide_wgrad_gpu.py's bound
EMU_TOL = 1e-6             # the fp32 statement of the summation order against fp64, on the CPU

CS = (1, 3, 4, 5, 8, 9, 12)            # each padded width (4, 8, 12) full and ragged
PS = (1, 49, 196, 256)                 # 49: scalar form, 196 / 256: 16-byte form, 1: one pixel per sample
BS = (1, 3, 33)                        # 33 x 49 = 1617 and 33 x 196 / 4 = 1617: no multiple of a block's 256 units
FORMS = ("plain", "presub", "presub_nodx", "nodb")

CASES = []
for _c in CS:
    for _p in PS:
        for _b in BS:
            CASES.append((_b, _c, _p, FORMS[len(CASES) % 4], 0))
MULTI_TRIP_C1 = (1025, 1, 256, "presub", 0)          # 65 600 units on 256 blocks: two trips, 256 slots: two rounds of the sum
CASES += [
    MULTI_TRIP_C1,
    (400, 3, 49, "plain", 0),                        # scalar form, 77 slots: two rounds
    (33, 12, 196, "presub", 2), (33, 8, 196, "plain", 2), (33, 4, 196, "nodb", 3),       # 16-byte form, 4 / 4 / 3 trips
    (33, 12, 49, "plain", 2), (33, 5, 49, "presub_nodx", 3), (33, 3, 49, "presub", 1),   # scalar form, 4 / 3 / 7 trips
    (33, 4, 256, "plain+unaligned", 0), (3, 9, 196, "presub+unaligned", 0), (5, 12, 256, "nodb+unaligned", 2),
]
REFUSED = [(4, 13, 49), (4, 0, 49), (4, 4, 0), (4, 64, 196)]


def case_id(case):
    B, C, P, form, cap = case
    return f"B{B}_C{C}_P{P}_{form}" + (f"_cap{cap}" if cap else "")


def aligned(case) -> bool:
    return "unaligned" not in case[3]


def wants(case):
    """(pre_sub, want_dx, want_db) of the case's form"""
    f = case[3].split("+")[0]
    return f.startswith("presub"), f != "presub_nodx", f != "nodb"


def inputs(case, device="cpu"):
    """x, dy [B, C, P, 1], W [C, C], pre_sub [C] | None -- seeded by the sizes.  dy and x - pre_sub are positive (dy, x in
    [0.5, 1.5), pre_sub in [-0.25, 0.25)): the bound is a fraction of max|ref|, and at C = 1 dW and db are ONE number each -- a
    sum of signed terms that happens to cancel would make that unit arbitrarily small for any fp32 summation, the numpy one
    of the CPU test included (three terms are enough).  W is signed: dx is held over B C P elements"""
    B, C, P, form, cap = case
    g = torch.Generator().manual_seed(1000 * B + 31 * C + P + 7 * cap)
    off = 0 if aligned(case) else 1
    n = B * C * P

    def tensor():
        buf = (0.5 + torch.rand(n + 4, generator=g)).to(device)
        return buf[off: off + n].view(B, C, P, 1)

    x, dy = tensor(), tensor()
    W = torch.randn(C, C, generator=g).to(device)
    ps = (0.5 * torch.rand(C, generator=g) - 0.25).to(device) if wants(case)[0] else None
    return x, dy, W, ps


def ref64(x, dy, W, ps):
    """dx [B, C, P, 1], dW [C, C], db [C] in fp64"""
    xd, dd = x.double().cpu().flatten(2), dy.double().cpu().flatten(2)
    if ps is not None:
        xd = xd - ps.double().cpu().view(1, -1, 1)
    dx = torch.einsum("ck,bcp->bkp", W.double().cpu(), dd).reshape(x.shape)
    return dx, torch.einsum("bcp,bkp->ck", dd, xd), dd.sum((0, 2))


def check(got, ref, what, tol=TOL):
    """every element within tol * max|ref|; returns the error in that unit"""
    scale = max(float(ref.abs().max()), 1e-30)
    err = float((got.double().cpu() - ref).abs().max())
    print(f"{what}: max|ref| {scale:.3e} err {err:.3e} ({err / scale:.2e} rel) bound {tol * scale:.3e}")
    assert bool(torch.isfinite(got).all()) and err <= tol * scale, (what, err, tol * scale)
    return err / scale


# ---- the kernel's summation order in numpy fp32 -----------------------------------------------------------------------------------
def _fma32(a, b, c):
    """fmaf on fp32 arrays: the product of two fp32 numbers is exact in fp64; the sum is rounded to fp64, then to fp32"""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def _sum_slots(part, plan):
    """usf_image_grad.hip partial_sum_block over the slots: four interleaved chains from 0.f, then ((0 + 1) + 2) + 3; above 64
    slots a first round over rows of `per` slots"""
    def rows_sum(p):
        chains = []
        for g in range(4):
            s = np.zeros(p.shape[1], np.float32)
            for i in range(g, p.shape[0], 4):
                s = s + p[i]
            chains.append(s)
        return ((chains[0] + chains[1]) + chains[2]) + chains[3]

    if plan["rounds"] == 2:
        per = plan["per"]
        part = np.stack([rows_sum(part[r * per: (r + 1) * per]) for r in range(plan["rows_used"])])
    return rows_sum(part)


def emulate(x, dy, ps, plan):
    """(dW [C, C], db [C]) as the kernel adds them, from the plan usf_channel_affine_bwd_variant answers: thread g = 256 block +
    t owns the units g, g + G, ... (G = 256 blocks; a unit = one pixel, or four of a row in the 16-byte form) and adds their
    pixels in ascending order (fmaf for dW, + for db); lanes l and l ^ 32, then ^ 16, .., ^ 1; the waves ((0 + 1) + 2) + 3; the slots as
    _sum_slots"""
    B, C, P = x.shape[0], x.shape[1], x.shape[2]
    px = 4 if plan["vec"] else 1
    G = plan["blocks"] * 256
    trips = plan["trips"]
    xs = x.cpu().numpy().astype(np.float32).reshape(B, C, P).transpose(0, 2, 1).reshape(B * P, C)      # [pixel, channel]
    ds = dy.cpu().numpy().astype(np.float32).reshape(B, C, P).transpose(0, 2, 1).reshape(B * P, C)
    if ps is not None:
        xs = xs - ps.cpu().numpy().astype(np.float32)[None, :]
    pad = trips * G * px - B * P                      # (units past the end: zeros add nothing -- fmaf(0, 0, s) == s)
    xs = np.concatenate([xs, np.zeros((pad, C), np.float32)]).reshape(trips, G, px, C)
    ds = np.concatenate([ds, np.zeros((pad, C), np.float32)]).reshape(trips, G, px, C)
    acc = np.zeros((G, C, C), np.float32)
    dbs = np.zeros((G, C), np.float32)
    for t in range(trips):
        for j in range(px):
            d, v = ds[t, :, j], xs[t, :, j]
            dbs = dbs + d
            acc = _fma32(d[:, :, None], v[:, None, :], acc)
    v = np.concatenate([acc.reshape(G, C * C), dbs], 1).reshape(plan["blocks"], 4, 64, C * C + C)
    for o in (32, 16, 8, 4, 2, 1):
        v = v[:, :, :o] + v[:, :, o:]
    v = v[:, :, 0]
    slots = ((v[:, 0] + v[:, 1]) + v[:, 2]) + v[:, 3]
    out = _sum_slots(slots, plan)
    return out[:C * C].reshape(C, C), out[C * C:]
