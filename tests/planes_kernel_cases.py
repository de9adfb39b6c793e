"""The two kernels of the planes pipeline -- gemm_planes_kernel<NPL, TN, F32OUT, SIDE> with its DEAD tile form
(usf_planes.hip: usf_gemm_planes_bf16x3 / usf_gemm_planes_side) and coupling_planes_kernel<NPL, NH, MODE, CTX, SIDE>
(usf_coupling_planes.hip: usf_coupling_planes / _ctx / _side) -- one launch at a time against fp64: the case tables, descriptor
builders that know nothing but the headers (the planes paragraph, usf_gemm_planes_desc and usf_coupling_planes_desc of
include/usflows_hip.h; usf_gemm_planes_side, usf_coupling_planes_ctx, usf_coupling_planes_side and the hidden_out / gate
paragraph of include/usflows_hip_internal.h), plane and weight-image encoders written out by hand (no engine packer, no
emulator), the layers in fp64 / fp32 on the CPU and the checkers.  Importable without a GPU:
tests/test_planes_kernels_cpu.py holds the tables and the checkers to account, tests/test_planes_kernels_gpu.py launches.

Buffers.  Every buffer has slack and a guard in front of and behind it.  A NaN with a payload of its own (bf16 / fp16 NaN bits in
plane buffers) sits wherever the contract keeps a launch from reading into a result or from writing: A blocks outside
[a_kb0, a_kb0 + nk), rows >= M of the last panel of A, residual, z, side and gate buffers, weight columns >= 32 nk up to ldw,
weight rows >= w_rows, the gap between weight planes, bias / post_mul beyond w_rows, the coupling's weight slack beyond 32 nk_p
resp. 256 columns, every chunk of C / z outside the written block range, every element of C_f32, base_part and the side buffer,
planes 1 and 2 of the gate buffers.  Zeros stand only where the header demands them: weight rows beyond the wanted outputs,
hidden padding, base_tab between N and its stride.

Bounds (the project's own rules, applied to EVERY element of every row < M):
 * GEMM: err <= max(4 err32, 6e-8 sqrt(32 nk)), errors relative to max |ref64| (test_gemm_planes_parity's rule)
 * coupling: err <= max(4 err32, 2e-6), errors relative to max |ref64| (test_coupling_planes_kernel_vs_reference_arithmetic's)
with err32 the same layer in fp32 on the CPU on the values the buffers actually hold.  Census cases and the exact columns of the
dead-tile scan cases are compared bit for bit."""
import collections
import contextlib
import functools
import math

import torch

FMT_BF16X3, FMT_F16X2 = 0, 1                          # include/usflows_hip.h: USF_PLANES_*
ACT_NONE, ACT_LEAKY_RELU, ACT_GATE = 0, 1, 2          # USF_ACT_*
BASE_LAPLACE, BASE_NORMAL = 0, 1                      # USF_BASE_*
GUARD = 2048                                          # bytes of NaN in front of and behind every plane / side buffer
EXTRA_ROWS = 3                                        # rows below M in row-major fp32 buffers


def ceil_to(n, m):
    return (n + m - 1) // m * m


def fmt_of(npl):
    return FMT_F16X2 if npl == 2 else FMT_BF16X3


def plane_dtype(npl):
    return torch.float16 if npl == 2 else torch.bfloat16


# ---- the planes layout, from the header's paragraph ---------------------------------------------------------------------------------
def slot_feature(s):
    """slot s = 8 g + u of a 32-feature block holds the block's feature 16 (u >> 2) + 4 g + (u & 3)"""
    g, u = s >> 3, s & 7
    return 16 * (u >> 2) + 4 * g + (u & 3)


_LANE = torch.arange(64)
_LANE_ROW = (_LANE & 15)[:, None]                                                           # line L = 16 g + j: row j of the panel
_LANE_FEAT = torch.tensor([[slot_feature(8 * (L >> 4) + u) for u in range(8)] for L in range(64)])
SLOT_ORDER = torch.tensor([slot_feature(s) for s in range(32)])                             # feature held by slot s


def to_chunks(logical):
    """logical [P, 16 npanels, 32 nkb] (P planes of 2-byte elements, or P = 1 fp32 plane: the side buffer) -> the chunk order of the
    header, flat: chunk(p, kb, q) holds 64 lines of 8 elements, line L = 16 g + j = row 16 p + j, slots 8 g .. 8 g + 7 of block kb"""
    P, R, F = logical.shape
    x = logical.view(P, R // 16, 16, F // 32, 32)
    ch = x[:, :, _LANE_ROW, :, _LANE_FEAT]                   # [64, 8, P, npanels, nkb]
    return ch.permute(3, 4, 2, 0, 1).contiguous().reshape(-1)


def from_chunks(flat, P, npanels, nkb):
    ch = flat.view(npanels, nkb, P, 64, 8)
    out = torch.empty(P, npanels, 16, nkb, 32, dtype=flat.dtype)
    out[:, :, _LANE_ROW, :, _LANE_FEAT] = ch.permute(3, 4, 2, 0, 1)
    return out.view(P, 16 * npanels, 32 * nkb)


def nan_bits16(n, npl, salt=0):
    """n quiet NaNs of the plane type as int16 bits, payloads cycling (a NaN that moved is another NaN)"""
    lin = torch.arange(n, dtype=torch.int64) + 7 * salt
    if npl == 2:
        return (0x7E00 + 1 + lin % 0x1FE).to(torch.int16)
    return (0x7FC0 + 1 + lin % 0x3E).to(torch.int16)


def nan_f32(n, salt=0):
    lin = torch.arange(n, dtype=torch.int64)
    return (0x7FC00000 + 1 + (lin + salt * 0x50001) % 0x3FFFFE).to(torch.int32).view(torch.float32)


def split_planes(x, npl):
    """the round-to-nearest residual split of fp32 x: [npl, ...] of the plane type (x == sum of the planes for bf16x3)"""
    dt = plane_dtype(npl)
    p0 = x.to(dt)
    r = x - p0.float()
    p1 = r.to(dt)
    if npl == 2:
        return torch.stack([p0, p1])
    return torch.stack([p0, p1, (r - p1.float()).to(dt)])


def plane_sum(planes):
    """the fp32 value a reader rebuilds from planes [npl, ...]: (p0 + p1) + p2"""
    v = planes[0].float() + planes[1].float()
    return v + planes[2].float() if planes.shape[0] == 3 else v


def bits16(t):
    return t.contiguous().view(torch.int16)


def bits32(t):
    return t.contiguous().view(torch.int32)


def planes_buffer(npl, M, nkb, blocks, salt):
    """a planes buffer of M rows and nkb blocks as logical int16 bits [npl, 16 npanels, 32 nkb]: NaN everywhere but the rows < M of
    `blocks` = {block index: fp32 values [M, 32]} (their split).  Returns (bits, values [M, 32 nkb] fp32 with NaN where poisoned)"""
    R = ceil_to(M, 16)
    bits = nan_bits16(npl * R * 32 * nkb, npl, salt).view(npl, R, 32 * nkb).clone()
    vals = torch.full((M, 32 * nkb), float("nan"))
    for kb, x in blocks.items():
        pl = split_planes(x.contiguous(), npl)
        bits[:, :M, 32 * kb: 32 * kb + 32] = bits16(pl)
        vals[:, 32 * kb: 32 * kb + 32] = plane_sum(pl)
    return bits, vals


def guarded(chunks16, npl, salt):
    """[guard | chunks | guard] as one int16 tensor; the buffer's address is GUARD bytes in"""
    g = GUARD // 2
    return torch.cat([nan_bits16(g, npl, salt + 1), chunks16, nan_bits16(g, npl, salt + 2)])


def unguarded(flat16):
    g = GUARD // 2
    return flat16[g: flat16.numel() - g]


def weight_image(planes, ld, extra_rows=2, gap=24, salt=0):
    """the weight image of the header from planes [npl, rows, K] given in LOGICAL feature order: column 32 kb + s of a row holds
    the weight of the feature at slot s of K block kb; row stride ld > K, extra_rows NaN rows behind the rows and `gap` NaN
    elements more between two planes.  Returns (flat int16 image, plane stride in elements)"""
    npl, rows, K = planes.shape
    assert ld % 8 == 0 and ld >= K and gap % 8 == 0 and K % 32 == 0
    cols = (torch.arange(K) // 32) * 32 + SLOT_ORDER[torch.arange(K) % 32]
    stride = (rows + extra_rows) * ld + gap
    flat = nan_bits16(npl * stride, npl, salt).clone()
    for q in range(npl):
        flat[q * stride: q * stride + rows * ld].view(rows, ld)[:, :K] = bits16(planes[q][:, cols])
    return flat, stride


def _seed(*ints):
    s = 24680
    for v in ints:
        s = (s * 1000003 + int(v) + 7) % (2 ** 31 - 1)
    return s


@contextlib.contextmanager
def knobs(pairs):
    """the library's tuning knobs `pairs` set for the block and put back afterwards"""
    from usflows_amd.config import config
    defaults = {"planes_skip_dead": 1, "planes_tn": 0, "planes_persist": 1, "coupling_act_max": 1, "coupling_descend": 1}
    old = [(name, config.get_lib(name, defaults[name])) for name, _ in pairs]
    for name, value in pairs:
        config.set_lib(name, value)
    try:
        yield
    finally:
        for name, value in old:
            config.set_lib(name, value)


def fake_ptr(name):
    """16-byte aligned addresses that are never read (the variant entry points are host-only)"""
    return 0x100000 + 0x100000 * (sum(name.encode()) % 251)


# =====================================================================================================================================
# GEMM on planes
# =====================================================================================================================================
# form: "planes" | "fp32" | "side".  n_out: planes / side: c_kbn, fp32: N.  res: None | "alias" | "sep".  base: None | "laplace" |
# "normal"; store: C_f32 given.  vec: 0 = ldc odd, 1 = C misaligned by 4 bytes, 2 = the 16-byte store path.  side: (side_kb0,
# side_kbn, both_kb0, both_kbn).  dead: None (the last 16 weight rows of the last column block are ordinary) | "zero" | "first" |
# "last" | "lastplane" | "negzero" (the dead-tile scan cases) -- kind: "table" | "dead" | "persist" | "scan" | "census"
GCase = collections.namedtuple("GCase", "kind npl tn form M a_nkb a_kb0 nk n_out w_rows c_nkb c_kb0 bias act slope res sign post_mul "
                                        "vec base store side dead idx")
G_M = [1, 15, 16, 17, 33, 255, 256, 257, 2049]
G_NK = [1, 2, 3, 4, 5, 6, 7]
G_ACTS = [(ACT_NONE, 0.0), (ACT_LEAKY_RELU, 0.01), (ACT_LEAKY_RELU, 0.0)]
# output blocks by TN: gemm_planes_tn takes the width that pads less, 5 on a tie
G_CKBN = {4: [1, 4, 7, 2, 6, 3, 8, 3, 2, 7], 5: [5, 9, 10, 13, 5, 9, 14, 10, 13, 9]}
G_N = {4: [77, 118, 33, 128, 1, 250, 204], 5: [150, 159, 160, 311, 275, 157, 148]}          # (none with 16 zero rows at the end of w_rows)
PERSIST_M, PERSIST_CKBN = 8193, {4: 28, 5: 35}
CENSUS_NK, CENSUS_M = 3, 33
KEPT = {3: [(2, 0), (1, 1), (0, 2), (1, 0), (0, 1), (0, 0)], 2: [(1, 0), (0, 1), (0, 0)]}          # (weight plane, activation plane)
DROPPED = {3: [(2, 1), (1, 2), (2, 2)], 2: [(1, 1)]}
CENSUS_SHIFT = 4                                      # plane q of a census operand holds integers times 2^(-4 q)


def gemm_tn(nblk):
    """gemm_planes_tn restated: the column-block width that pads nblk 32-feature blocks less, 5 on a tie"""
    pad5, pad4 = ceil_to(nblk, 5) - nblk, ceil_to(nblk, 4) - nblk
    return 4 if pad4 < pad5 else 5


def _g(kind, npl, tn, form, i, M, nk, n_out, **kw):
    f = dict(a_kb0=i % 3, bias=True, act=ACT_NONE, slope=0.0, res=None, sign=1.0, post_mul=False, vec=2, base=None, store=True,
             side=None, dead=None, c_kb0=0, c_nkb=None, w_rows=None)
    f.update(kw)
    a_nkb = f["a_kb0"] + nk + (i % 2)
    if form == "fp32":
        c_nkb, c_kb0 = 0, 0
        w_rows = f["w_rows"] or (ceil_to(n_out, 4) if i % 2 else ceil_to(n_out, 32))
    else:
        c_kb0 = f["c_kb0"]
        c_nkb = f["c_nkb"] or c_kb0 + n_out + 1
        w_rows = f["w_rows"] or 32 * n_out + 4 * (i % 2)
    return GCase(kind, npl, tn, form, M, a_nkb, f["a_kb0"], nk, n_out, w_rows, c_nkb, c_kb0, f["bias"], f["act"], f["slope"], f["res"],
                 f["sign"], f["post_mul"], f["vec"], f["base"], f["store"], f["side"], f["dead"], i)


def _build_gemm_cases():
    cases = []
    for npl in (3, 2):
        for tn in (4, 5):
            ck, ns = G_CKBN[tn], G_N[tn]
            rows = []          # (form, options); M, nk, the output width, a_kb0 and the slack cycle with the row's index
            for res, sign in [(None, 1.0), ("alias", 1.0), ("alias", -1.0), ("sep", 1.0), ("sep", -1.0), (None, 1.0)]:
                rows.append(("planes", dict(res=res, sign=sign)))
            rows += [("fp32", dict(vec=2, post_mul=True)), ("fp32", dict(vec=0, bias=False)), ("fp32", dict(vec=1, post_mul=True)),
                     ("fp32", dict(base="laplace", store=True, vec=2)), ("fp32", dict(base="normal", store=False)),
                     ("fp32", dict(base="normal", store=True, vec=0)), ("fp32", dict(base="laplace", store=False, bias=False))]
            # side ranges as fractions of c_kbn: all / prefix / interior / suffix; both: empty / partial / full / partial
            rows += [("side", dict(side="all")), ("side", dict(side="prefix")), ("side", dict(side="interior")),
                     ("side", dict(side="suffix"))]
            for i, (form, opt) in enumerate(rows):
                j = i + 2 * tn + npl
                act, slope = G_ACTS[j % 3]
                n_out = ns[i % 7] if form == "fp32" else ck[i % 10]
                opt = dict(opt)
                opt.setdefault("bias", i % 5 != 4)
                if form != "fp32":
                    opt["c_kb0"] = i % 2
                if form == "side":
                    n = n_out
                    kind = opt["side"]
                    if kind == "all":
                        opt["side"] = (0, n, 0, 0)
                    elif kind == "prefix":
                        opt["side"] = (0, max(1, n // 2), 0, 1)
                    elif kind == "interior":
                        opt["side"] = (1, n - 2, 1, n - 2) if n >= 3 else (0, n, 0, n)
                    else:
                        opt["side"] = (n // 2, n - n // 2, n - 1, 1)
                cases.append(_g("table", npl, tn, form, i, G_M[j % 9], G_NK[j % 7], n_out, act=act, slope=slope, **opt))
            # the DEAD form of every (form) -- the last column block wholly inside w_rows, its last 16 weight rows all-zero bits
            wide = 32 * tn
            cases.append(_g("dead", npl, tn, "planes", 20, 257, 3, tn, dead="zero", w_rows=wide, res="alias", sign=-1.0,
                            act=ACT_LEAKY_RELU, slope=0.01))
            cases.append(_g("dead", npl, tn, "fp32", 21, 33, 2, wide - 10, dead="zero", w_rows=wide, post_mul=True, base="laplace"))
            cases.append(_g("dead", npl, tn, "side", 22, 17, 5, 2 * tn, dead="zero", w_rows=2 * wide, side=(tn, tn, 2 * tn - 1, 1)))
            # the dead-tile scan: rows that are not quite dead, and a -0 among them
            for k, dead in enumerate(["first", "last", "lastplane", "negzero"]):
                cases.append(_g("scan", npl, tn, "planes", 30 + k, 33, 3, tn, dead=dead, w_rows=wide, bias=(dead != "lastplane"), a_kb0=1))
            # six-product census: fp32 output, no bias, no activation
            cases.append(_g("census", npl, tn, "fp32", 40, CENSUS_M, CENSUS_NK, wide, bias=False, a_kb0=1))
    # a persistent block's second tile: 40 x 7 = 280 virtual blocks against 256 CUs
    cases.append(_g("persist", 3, 4, "planes", 50, PERSIST_M, 1, PERSIST_CKBN[4], a_kb0=0, c_nkb=PERSIST_CKBN[4]))
    cases.append(_g("persist", 2, 5, "planes", 51, PERSIST_M, 1, PERSIST_CKBN[5], a_kb0=0, c_nkb=PERSIST_CKBN[5], act=ACT_LEAKY_RELU,
                    slope=0.01))
    return cases


GEMM_CASES = _build_gemm_cases()


def gemm_case_id(c):
    out = f"N{c.n_out}" if c.form == "fp32" else f"c{c.n_out}at{c.c_kb0}of{c.c_nkb}"
    return (f"{c.kind}-npl{c.npl}-tn{c.tn}-{c.form}-M{c.M}-k{c.nk}at{c.a_kb0}of{c.a_nkb}-{out}-w{c.w_rows}-{'b' if c.bias else 'nob'}"
            f"-act{c.act}s{c.slope}-res_{c.res}{c.sign:+.0f}{'-pm' if c.post_mul else ''}-v{c.vec}-base_{c.base}{'' if c.store else '-nostore'}"
            + (f"-side{'_'.join(map(str, c.side))}" if c.side else "") + (f"-{c.dead}" if c.dead else ""))


def gemm_nblk(c):
    return ceil_to(c.n_out, 32) // 32 if c.form == "fp32" else c.n_out


def gemm_cols(c):
    """output features a launch computes and stores: N (fp32 output) or 32 c_kbn"""
    return c.n_out if c.form == "fp32" else 32 * c.n_out


def gemm_grid(c):
    """(nbm, nbn, nvb) by launch_planes' rule: 256-row panel groups, column blocks, virtual blocks"""
    tn = gemm_tn(gemm_nblk(c))
    nbm = ceil_to(ceil_to(c.M, 16) // 16, 16) // 16
    nbn = ceil_to(gemm_nblk(c), tn) // tn
    return nbm, nbn, ceil_to(nbm, 8) * nbn


def gemm_variant_code(c):
    """usf_gemm_planes_variant restated: 5000 + 10 TN + (1: fp32 output)"""
    return 5000 + 10 * gemm_tn(gemm_nblk(c)) + (1 if c.form == "fp32" else 0)


def gemm_dead(c):
    """whether the launch takes the DEAD tile form, from the image itself: the last column block wholly inside w_rows and the
    last 16 of its rows all-zero bits in every plane over the K range"""
    tn = gemm_tn(gemm_nblk(c))
    end = gemm_grid(c)[1] * 32 * tn
    if end > c.w_rows:
        return False
    pl = gemm_prepared(c)["W_planes"]
    return bool((bits16(pl[:, end - 16: end]) == 0).all())


def gemm_instantiation(c):
    """(NPL, TN, form, DEAD)"""
    return c.npl, gemm_tn(gemm_nblk(c)), c.form, int(gemm_dead(c))


def _act(v, act, slope):
    return torch.where(v > 0, v, v * slope) if act == ACT_LEAKY_RELU else v


def census_products(p):
    """every plane product of a census case in fp64: {(weight plane i, activation plane j): [M, N]}"""
    A, W = p["A_planes"], p["W_planes"]
    return {(i, j): A[j].double() @ W[i].double().t() for i in range(W.shape[0]) for j in range(A.shape[0])}


def gemm_forward(c, p, dtype, defect=None):
    """the layer in `dtype` on the values the buffers hold, in the header's order: dict(C=[M, cols], part=[M, nbn] or None)"""
    W = p["W_eff"]
    bias = p["bias"][: c.w_rows] if c.bias else None
    if defect == "no_dead_rows":
        W = W.clone()
        end = gemm_grid(c)[1] * 32 * c.tn
        W[end - 16: end] = 0
    if defect == "bias_shifted" and bias is not None:
        bias = torch.roll(bias, 16)
    cols = gemm_cols(c)
    if c.kind == "census":
        prods = census_products(p)
        keep = list(KEPT[c.npl])
        if defect == "drop_product":
            keep = keep[1:]
        if defect == "add_product":
            keep = keep + DROPPED[c.npl][:1]
        v = sum(prods[k] for k in keep).to(dtype)
    else:
        v = p["A_eff"].to(dtype) @ W[:cols].to(dtype).t()
    if bias is not None:
        v = v + bias[:cols].to(dtype)
    v = _act(v, c.act, c.slope)
    if c.res:
        v = p["R_eff"].to(dtype) + (-c.sign if defect == "res_sign" else c.sign) * v
    if c.post_mul:
        v = v * p["post_mul"][:cols].to(dtype)
    part = None
    if c.base:
        tab, st = p["base_tab"], p["tab_stride"]
        d = (v - tab[:cols].to(dtype)) * tab[st: st + cols].to(dtype)
        term = tab[2 * st: 2 * st + cols].to(dtype) - (d.abs() if c.base == "laplace" else 0.5 * d * d)
        bn = 32 * c.tn
        nbn = gemm_grid(c)[1]
        part = torch.stack([term[:, j * bn: (j + 1) * bn].sum(1) for j in range(nbn)], 1)
    return dict(C=v, part=part)


def _rel_bound(ref64, ref32, floor):
    scale = ref64.abs().max().item() or 1.0
    err32 = (ref32.double() - ref64).abs().max().item() / scale
    return scale, err32, max(4 * err32, floor)


@functools.lru_cache(maxsize=3)
def gemm_prepared(c, perm_seed=None):
    """host buffers and references of a case; perm_seed: the same case with the rows of A and the residual permuted"""
    npl, M, nk, K = c.npl, c.M, c.nk, 32 * c.nk
    g = torch.Generator().manual_seed(_seed(npl, c.tn, M, nk, c.n_out, c.idx, len(c.form)))
    R = ceil_to(M, 16)
    cols = gemm_cols(c)
    p = {}
    perm = torch.randperm(M, generator=torch.Generator().manual_seed(perm_seed)) if perm_seed is not None else torch.arange(M)
    p["perm"] = perm
    # ---- A: the K range's blocks hold values, everything else NaN
    if c.kind == "census":
        ints = [torch.randint(1, 3, (M, K), generator=g) * (2 * torch.randint(0, 2, (M, K), generator=g) - 1) for _ in range(npl)]
        A_planes = torch.stack([(ints[q].float() * 2.0 ** (-CENSUS_SHIFT * q)).to(plane_dtype(npl)) for q in range(npl)])
    else:
        X = torch.randn(M, K, generator=g) * 3
        if c.dead == "lastplane":
            X = torch.randint(-8, 9, (M, K), generator=g).float() / 4          # exactly representable in plane 0
        A_planes = split_planes(X, npl)
    A_planes = A_planes[:, perm]
    A_bits = nan_bits16(npl * R * 32 * c.a_nkb, npl, 1).view(npl, R, 32 * c.a_nkb).clone()
    A_bits[:, :M, 32 * c.a_kb0: 32 * c.a_kb0 + K] = bits16(A_planes)
    p["A_planes"], p["A_eff"] = A_planes, plane_sum(A_planes)
    p["A"] = guarded(to_chunks(A_bits), npl, 2)
    # ---- W: rows beyond the wanted outputs zero; the dead-tile forms of the last 16 rows of the last column block
    if c.kind == "census":
        ints = [torch.randint(1, 3, (c.w_rows, K), generator=g) * (2 * torch.randint(0, 2, (c.w_rows, K), generator=g) - 1) for _ in range(npl)]
        W_planes = torch.stack([(ints[q].float() * 2.0 ** (-CENSUS_SHIFT * q)).to(plane_dtype(npl)) for q in range(npl)])
    else:
        W = torch.randn(c.w_rows, K, generator=g) / math.sqrt(K)
        W[cols:] = 0
        if c.dead:
            end = gemm_grid(c)[1] * 32 * c.tn
            assert end <= c.w_rows
            W[end - 16: end] = 0
            if c.dead == "first":
                W[end - 16, 0] = 0.7371
            elif c.dead == "last":
                W[end - 1, K - 1] = -0.6113
            elif c.dead == "negzero":
                W[end - 13, 5] = -0.0
        W_planes = split_planes(W, npl)
        if c.dead == "lastplane":
            W_planes[npl - 1, end - 1, K - 1] = 2.0 ** -10
    p["W_planes"], p["W_eff"] = W_planes, plane_sum(W_planes)
    ldw = K + 8 * (1 + c.idx % 2)
    p["W"], p["w_plane_stride"] = weight_image(W_planes, ldw, salt=3)
    p["ldw"] = ldw
    if c.bias:
        p["bias"] = torch.cat([torch.randn(c.w_rows, generator=g), nan_f32(8, 4)])
    if c.post_mul:
        pm = (torch.rand(c.w_rows, generator=g) + 0.5) * torch.where(torch.rand(c.w_rows, generator=g) < 0.5, -1.0, 1.0)
        p["post_mul"] = torch.cat([pm, nan_f32(8, 5)])
    # ---- outputs as they stand before the launch
    if c.form == "fp32":
        ldc = {0: cols + (1 if cols % 2 == 0 else 2), 1: ceil_to(cols, 4) + 4, 2: ceil_to(cols, 4) + 4}[c.vec]
        p["ldc"], p["c_off"] = ldc, (1 if c.vec == 1 else 0)
        p["C0"] = nan_f32((M + EXTRA_ROWS) * ldc + 4, 6)
        if c.base:
            st = ceil_to(cols, 4) + 4 * (c.idx % 2)
            tab = torch.zeros(3 * st)
            scale = torch.rand(cols, generator=g) + 0.5
            tab[:cols] = torch.randn(cols, generator=g)
            tab[st: st + cols] = 1.0 / scale
            tab[2 * st: 2 * st + cols] = -torch.log(2 * scale) if c.base == "laplace" else -torch.log(scale) - 0.5 * math.log(2 * math.pi)
            p["base_tab"], p["tab_stride"] = torch.cat([tab, nan_f32(8, 7)]), st
            p["part0"] = nan_f32((M + EXTRA_ROWS) * 8, 8)
    else:
        lo, hi = 32 * c.c_kb0, 32 * c.c_kb0 + cols
        C_bits = nan_bits16(npl * R * 32 * c.c_nkb, npl, 9).view(npl, R, 32 * c.c_nkb).clone()
        if c.res:
            Rv = (torch.randn(M, cols, generator=g) * 2)[perm]
            R_planes = split_planes(Rv, npl)
            p["R_eff"] = plane_sum(R_planes)
            if c.res == "alias":
                C_bits[:, :M, lo:hi] = bits16(R_planes)
            else:
                R_bits = nan_bits16(npl * R * 32 * c.c_nkb, npl, 10).view(npl, R, 32 * c.c_nkb).clone()
                R_bits[:, :M, lo:hi] = bits16(R_planes)
                p["Rbuf"] = guarded(to_chunks(R_bits), npl, 11)
        p["C0_bits"] = C_bits
        p["C0"] = guarded(to_chunks(C_bits), npl, 12)
        if c.form == "side":
            p["S0"] = torch.cat([nan_f32(GUARD // 4, 13), nan_f32((R // 16) * c.side[1] * 512, 14), nan_f32(GUARD // 4, 15)])
    # ---- references
    r64, r32 = gemm_forward(c, p, torch.float64), gemm_forward(c, p, torch.float32)
    floor = 6e-8 * math.sqrt(32 * nk)
    p["ref64"], p["ref32"] = r64, r32
    p["scale"], p["err32"], p["bound"] = _rel_bound(r64["C"], r32["C"], floor)
    if c.base:
        p["part_scale"], p["part_err32"], p["part_bound"] = _rel_bound(r64["part"], r32["part"], floor)
    return p


GEMM_INPUTS = ["A", "W", "bias", "post_mul", "Rbuf", "base_tab"]          # buffers a launch only reads


def gemm_exact_cols(c):
    """columns compared bit for bit: all of a census case; the not-quite-dead rows' output of the `lastplane` scan case"""
    if c.kind == "census":
        return slice(0, gemm_cols(c))
    if c.dead == "lastplane":
        end = gemm_grid(c)[1] * 32 * c.tn
        return slice(end - 16, end)
    return None


def gemm_blocks(c):
    """for every output block kbo < c_kbn: (written as planes, written to the side buffer)"""
    out = []
    for kbo in range(c.n_out):
        if c.form == "side":
            s0, sn, b0, bn = c.side
            to_side = s0 <= kbo < s0 + sn
            out.append((not to_side or b0 <= kbo < b0 + bn, to_side))
        else:
            out.append((True, False))
    return out


def gemm_as_launch(c, out, pad_rows=float("nan"), p=None):
    """the buffers as a launch that computes out = dict(C=[M, cols], part=...) would leave them: dict(C, S, part, flag)"""
    p = p or gemm_prepared(c)
    M, npl, R = c.M, c.npl, ceil_to(c.M, 16)
    got = dict(flag=0)
    v = out["C"].to(torch.float32)
    if c.form == "fp32":
        C = p["C0"].clone()
        if c.store:
            C[p["c_off"]: p["c_off"] + (M + EXTRA_ROWS) * p["ldc"]].view(M + EXTRA_ROWS, p["ldc"])[:M, : c.n_out] = v
        got["C"] = C
        if c.base:
            part = p["part0"].clone()
            part.view(-1, 8)[:M, : out["part"].shape[1]] = out["part"].to(torch.float32)
            got["part"] = part
        return got
    bits = p["C0_bits"].clone()
    side = None
    if c.form == "side":
        side = bits32(unguarded_f32(p["S0"])).clone()
        side_l = from_chunks(side, 1, R // 16, c.side[1])
    full = torch.full((R, v.shape[1]), pad_rows)
    full[:M] = v
    for kbo, (to_planes, to_side) in enumerate(gemm_blocks(c)):
        blk = full[:, 32 * kbo: 32 * kbo + 32]
        if to_side:
            sv = plane_sum(split_planes(blk, npl)) if npl == 2 else blk
            side_l[0, :, 32 * (kbo - c.side[0]): 32 * (kbo - c.side[0]) + 32] = bits32(sv)
        if to_planes:
            bits[:, :, 32 * (c.c_kb0 + kbo): 32 * (c.c_kb0 + kbo) + 32] = bits16(split_planes(blk.contiguous(), npl))
    got["C"] = guarded(to_chunks(bits), npl, 12)
    if side is not None:
        S = p["S0"].clone()
        S[GUARD // 4: S.numel() - GUARD // 4] = to_chunks(side_l).view(torch.float32)
        got["S"] = S
    return got


def unguarded_f32(flat):
    g = GUARD // 4
    return flat[g: flat.numel() - g]


def _same_split(v, planes):
    """planes [npl, ...] are the round-to-nearest residual split of their fp32 sum v (a -0 whose planes sum to +0 counts as 0)"""
    if planes.shape[0] == 2:
        return True          # (two fp16 planes: splitting the 22-bit sum again may round a tie the other way -- nothing to hold them to)
    return bool((split_planes(v, 3).float() == planes.float()).all())


def _max_rel(got, ref64, scale):
    err = (got.double() - ref64).abs() / scale
    return torch.where(torch.isnan(err), torch.full_like(err, float("inf")), err)


def gemm_check(c, got, p=None):
    """(violations, figures): an empty list of violations = the launch is right.  got: dict(C, S, part, flag) of CPU tensors shaped
    like the case's C0 / S0 / part0.  figures: dict(err, err32, bound) of the worst output"""
    p = p or gemm_prepared(c)
    M, npl, R, cols = c.M, c.npl, ceil_to(c.M, 16), gemm_cols(c)
    bad = []
    exact = gemm_exact_cols(c)
    r64 = p["ref64"]["C"]
    fig = dict(err=0.0, err32=p["err32"], bound=p["bound"])

    def values(name, v, ref=r64, scale=p["scale"], bound=p["bound"], ex=exact):
        if torch.isnan(v).any():
            bad.append(f"{name}: NaN in {int(torch.isnan(v).sum())} elements of the rows < M")
        err = _max_rel(v, ref, scale)
        fig["err"] = max(fig["err"], err.max().item() * (p["bound"] / bound))
        if err.max().item() > bound:
            r, k = divmod(int(err.argmax()), v.shape[1])
            bad.append(f"{name}: error {err.max().item():.3e} above the bound {bound:.3e} at row {r}, column {k}")
        if ex is not None and not torch.equal(bits32(v[:, ex].float()), bits32(ref[:, ex].float())):
            bad.append(f"{name}: the exact columns differ from the reference in {int((v[:, ex].double() != ref[:, ex]).sum())} elements")

    if int(got.get("flag", 0)) != 0:
        bad.append("range_flag raised")
    if c.form == "fp32":
        C, C0 = got["C"], p["C0"]
        if C.shape != C0.shape:
            return [f"C has shape {tuple(C.shape)}"], fig
        lo, n = p["c_off"], (M + EXTRA_ROWS) * p["ldc"]
        moved = bits32(C) != bits32(C0)
        if c.store:
            values("C_f32", C[lo: lo + n].view(-1, p["ldc"])[:M, :cols])
            moved[lo: lo + n].view(-1, p["ldc"])[:M, :cols] = False
        if moved.any():
            bad.append(f"C_f32: {int(moved.sum())} elements outside C[:M, :N] changed, the first at flat index {int(moved.to(torch.uint8).argmax())}")
        if c.base:
            nbn = gemm_grid(c)[1]
            part = got["part"]
            values("base_part", part.view(-1, 8)[:M, :nbn], p["ref64"]["part"], p["part_scale"], p["part_bound"], None)
            moved = bits32(part) != bits32(p["part0"])
            moved.view(-1, 8)[:M, :nbn] = False
            if moved.any():
                bad.append(f"base_part: {int(moved.sum())} elements outside [:M, :nbn] changed")
        return bad, fig
    C, C0 = got["C"], p["C0"]
    if C.shape != C0.shape:
        return [f"C has shape {tuple(C.shape)}"], fig
    g = GUARD // 2
    if not torch.equal(C[:g], C0[:g]) or not torch.equal(C[-g:], C0[-g:]):
        bad.append("C_planes: a guard changed")
    bits = from_chunks(unguarded(C), npl, R // 16, c.c_nkb)
    keep = torch.ones(32 * c.c_nkb, dtype=torch.bool)
    side_l = None
    if c.form == "side":
        S, S0 = got["S"], p["S0"]
        gs = GUARD // 4
        if not torch.equal(bits32(S[:gs]), bits32(S0[:gs])) or not torch.equal(bits32(S[-gs:]), bits32(S0[-gs:])):
            bad.append("side: a guard changed")
        side_l = from_chunks(unguarded_f32(S), 1, R // 16, c.side[1])[0]
    for kbo, (to_planes, to_side) in enumerate(gemm_blocks(c)):
        sl = slice(32 * (c.c_kb0 + kbo), 32 * (c.c_kb0 + kbo) + 32)
        rs = slice(32 * kbo, 32 * kbo + 32)
        ex = None
        if exact is not None and exact.start < rs.stop and exact.stop > rs.start:
            ex = slice(max(exact.start, rs.start) - rs.start, min(exact.stop, rs.stop) - rs.start)
        pv = None
        if to_planes:
            keep[sl] = False
            pl = bits[:, :M, sl].contiguous().view(plane_dtype(npl))
            pv = plane_sum(pl)
            values(f"C_planes block {kbo}", pv, r64[:, rs], ex=ex)
            if not torch.isnan(pv).any() and not _same_split(pv, pl):
                bad.append(f"C_planes block {kbo}: the planes are not the split of their sum")
        if to_side:
            sv = side_l[:M, 32 * (kbo - c.side[0]): 32 * (kbo - c.side[0]) + 32]
            values(f"side block {kbo}", sv, r64[:, rs], ex=ex)
            if pv is not None and not bool((sv == pv).all()):
                bad.append(f"side block {kbo}: the side values are not what the planes hold")
            if npl == 2 and not torch.equal(bits32(plane_sum(split_planes(sv.contiguous(), 2))), bits32(sv.contiguous())) and not torch.isnan(sv).any():
                bad.append(f"side block {kbo}: an f16x2 side value is not the sum of two fp16 planes")
    if not torch.equal(bits[:, :, keep], p["C0_bits"][:, :, keep]):
        n = int((bits[:, :, keep] != p["C0_bits"][:, :, keep]).sum())
        bad.append(f"C_planes: {n} elements of blocks outside the written range changed")
    return bad, fig


def gemm_descriptor(c, ptr, desc_type, p=None):
    """(usf_gemm_planes_desc, side arguments or None) of a case; ptr(name) gives the address of the buffer `name` as the launch
    must see it (guards and the fp32 misalignment already skipped)"""
    p = p or gemm_prepared(c)
    d = desc_type()
    d.A, d.a_nkb, d.a_kb0, d.nk = ptr("A"), c.a_nkb, c.a_kb0, c.nk
    d.W_planes, d.ldw, d.w_plane_stride, d.w_rows = ptr("W"), p["ldw"], p["w_plane_stride"], c.w_rows
    if c.bias:
        d.bias = ptr("bias")
    if c.post_mul:
        d.post_mul = ptr("post_mul")
    d.M, d.res_sign, d.slope, d.act, d.format = c.M, c.sign, c.slope, c.act, fmt_of(c.npl)
    d.range_flag = ptr("flag")
    side = None
    if c.form == "fp32":
        if c.store:
            d.C_f32 = ptr("C")
        d.ldc, d.N = p["ldc"], c.n_out
        if c.base:
            d.base_tab, d.base_tab_stride, d.base_part = ptr("base_tab"), p["tab_stride"], ptr("part")
            d.base = BASE_LAPLACE if c.base == "laplace" else BASE_NORMAL
    else:
        d.C_planes, d.c_nkb, d.c_kb0, d.c_kbn = ptr("C"), c.c_nkb, c.c_kb0, c.n_out
        if c.res:
            d.residual = ptr("C") if c.res == "alias" else ptr("Rbuf")
        if c.form == "side":
            side = (ptr("S"),) + tuple(c.side)
    return d, side


# =====================================================================================================================================
# fused coupling on planes
# =====================================================================================================================================
# mode: "plain" | "ctx" | "side" | "hout" (MODE 1) | "hout_ctx" (MODE 1 + CTX) | "gate" (MODE 2).  geo: "front" (conditioning blocks,
# a poisoned gap block, transformed blocks), "behind" (transformed blocks first), "shared" (the ranges share a straddling block)
CCase = collections.namedtuple("CCase", "npl nh mode M geo nk_p nk_t hidden act slope sign ctx_stride idx")
C_M = [1, 15, 16, 17, 127, 128, 129, 250, 1025]
C_NKP, C_NKT = [1, 2, 3, 5], [1, 2, 3]
C_WIDTHS = [256, 200, 17, 1]
C_ACTS = [(ACT_LEAKY_RELU, 0.01), (ACT_LEAKY_RELU, 0.0), (ACT_LEAKY_RELU, 1.0), (ACT_LEAKY_RELU, 1.5), (ACT_LEAKY_RELU, -0.5),
          (ACT_LEAKY_RELU, -0.0), (ACT_NONE, 0.0)]
C_GEOS = ["front", "behind", "shared"]
SHARED_SPLIT = 20                                     # the straddling block: conditioning features [0, 20), transformed [20, 32)
C_INSTANCES = ([(npl, nh, mode) for mode in ("plain", "ctx", "side") for npl in (3, 2) for nh in (1, 2, 3)]
               + [(3, nh, mode) for mode in ("hout", "hout_ctx", "gate") for nh in (1, 2)])
C_PER_INSTANCE = 3


def _build_coupling_cases():
    cases, i = [], 0
    for npl, nh, mode in C_INSTANCES:
        for rep in range(C_PER_INSTANCE):
            act, slope = C_ACTS[i % 7]
            if mode == "gate":
                act, slope = ACT_GATE, (0.01, 0.0, 1.5)[rep]
            hidden = tuple(C_WIDTHS[(i + l) % 4] for l in range(nh))
            cases.append(CCase(npl, nh, mode, C_M[i % 9], C_GEOS[(i + i // 3) % 3], C_NKP[i % 4], C_NKT[(i + i // 9) % 3], hidden, act, slope,
                               1.0 if (i // 2) % 2 == 0 else -1.0, rep % 2 if "ctx" in mode else 0, i))
            i += 1
    return cases


COUPLING_CASES = _build_coupling_cases()


def coupling_case_id(c):
    return (f"npl{c.npl}-nh{c.nh}-{c.mode}-M{c.M}-{c.geo}-p{c.nk_p}-t{c.nk_t}-h{'x'.join(map(str, c.hidden))}-act{c.act}s{c.slope}"
            f"-{'fwd' if c.sign > 0 else 'bwd'}-cs{c.ctx_stride}")


def coupling_variant_code(c):
    """usf_coupling_planes_variant restated: 70000 + 1000 NPL + 100 NH + 10 MODE + 2 CTX + SIDE"""
    mode = {"plain": 0, "ctx": 0, "side": 0, "hout": 1, "hout_ctx": 1, "gate": 2}[c.mode]
    return 70000 + 1000 * c.npl + 100 * c.nh + 10 * mode + 2 * int("ctx" in c.mode) + int(c.mode == "side")


def coupling_geometry(c):
    """dict(z_nkb, kb_p0, kb_t0, p_cols, t_cols): block ranges and the logical columns of z that are conditioning / transformed
    features; z has more blocks than the layer uses"""
    if c.geo == "front":
        kb_p0 = 1
        kb_t0 = kb_p0 + c.nk_p + 1                                                  # a poisoned gap block between the ranges
    elif c.geo == "behind":
        kb_t0 = 0
        kb_p0 = c.nk_t
    else:
        kb_p0 = 1
        kb_t0 = kb_p0 + c.nk_p - 1                                                  # the last conditioning block is the first transformed
    z_nkb = max(kb_p0 + c.nk_p, kb_t0 + c.nk_t) + 2
    p_cols = torch.zeros(32 * z_nkb, dtype=torch.bool)
    t_cols = torch.zeros(32 * z_nkb, dtype=torch.bool)
    p_cols[32 * kb_p0: 32 * (kb_p0 + c.nk_p)] = True
    t_cols[32 * kb_t0: 32 * (kb_t0 + c.nk_t)] = True
    if c.geo == "shared":
        p_cols[32 * kb_t0 + SHARED_SPLIT: 32 * kb_t0 + 32] = False
        t_cols[32 * kb_t0: 32 * kb_t0 + SHARED_SPLIT] = False
    return dict(z_nkb=z_nkb, kb_p0=kb_p0, kb_t0=kb_t0, p_cols=p_cols, t_cols=t_cols)


def coupling_forward(c, p, dtype, defect=None):
    """the layer in `dtype` on the values the buffers hold: dict(t=[M, 32 nk_t] new values of the transformed blocks,
    hidden=[activations of every hidden layer, [M, 256]])"""
    geo = coupling_geometry(c)
    x = p["z_eff"][:, 32 * geo["kb_p0"]: 32 * (geo["kb_p0"] + c.nk_p)].to(dtype)
    hidden = []
    h = x
    for l in range(c.nh):
        W, b = p["W_eff"][l], p["b"][l][:256]
        if defect == "bias_shifted" and l == 0:
            b = torch.roll(b, 16)
        h = h @ W.to(dtype).t() + b.to(dtype)
        if l == 0 and "ctx" in c.mode:
            ctx = p["ctx"][:c.M] if c.ctx_stride == 1 else p["ctx"][:1].expand(c.M)
            h = h + p["b_ctx"].to(dtype) + ctx.to(dtype)[:, None] * p["w_ctx"].to(dtype)[None, :]
        if c.mode == "gate":
            h = h * torch.where(p["gate_eff"][l] > 0, 1.0, c.slope).to(dtype)
        elif c.act == ACT_LEAKY_RELU:
            h = torch.where(h > 0, h, h * c.slope)
        hidden.append(h)
    out = h @ p["W_eff"][c.nh].to(dtype).t() + p["b"][c.nh][: 32 * c.nk_t].to(dtype)
    zt = p["z_eff"][:, 32 * geo["kb_t0"]: 32 * (geo["kb_t0"] + c.nk_t)].to(dtype)
    return dict(t=zt + (-c.sign if defect == "res_sign" else c.sign) * out, hidden=hidden)


def _cw_image(W, npl, ld, salt):
    planes = split_planes(W, npl)
    flat, stride = weight_image(planes, ld, salt=salt)
    return planes, flat, stride


@functools.lru_cache(maxsize=3)
def coupling_prepared(c, perm_seed=None):
    npl, M, nh = c.npl, c.M, c.nh
    geo = coupling_geometry(c)
    z_nkb, kb_p0, kb_t0 = geo["z_nkb"], geo["kb_p0"], geo["kb_t0"]
    g = torch.Generator().manual_seed(_seed(M, c.nk_p, c.nk_t, c.idx, *c.hidden))
    R = ceil_to(M, 16)
    perm = torch.randperm(M, generator=torch.Generator().manual_seed(perm_seed)) if perm_seed is not None else torch.arange(M)
    p = dict(perm=perm)
    used = sorted(set(range(kb_p0, kb_p0 + c.nk_p)) | set(range(kb_t0, kb_t0 + c.nk_t)))
    X = (torch.randn(M, 32 * z_nkb, generator=g) * 2)[perm]
    z_bits, z_vals = planes_buffer(npl, M, z_nkb, {kb: X[:, 32 * kb: 32 * kb + 32] for kb in used}, 20)
    p["z0_bits"], p["z_eff"] = z_bits, z_vals
    p["z0"] = guarded(to_chunks(z_bits), npl, 21)
    # ---- weights: hidden widths zero-padded to 256; the other set's features of the shared block have zero weights / rows
    Kin = 32 * c.nk_p
    dims = [Kin] + list(c.hidden) + [32 * c.nk_t]
    Ws, bs = [], []
    for l in range(nh + 1):
        fan = dims[l]
        rows, colsn = (256 if l < nh else 32 * c.nk_t), (Kin if l == 0 else 256)
        W = torch.zeros(rows, colsn)
        b = torch.zeros(rows)
        n_r, n_c = dims[l + 1], dims[l]
        W[:n_r, :n_c] = torch.randn(n_r, n_c, generator=g) / math.sqrt(fan)
        b[:n_r] = torch.randn(n_r, generator=g) * 0.1
        if c.mode == "gate":
            b[:] = 0                                    # the backward chain: zero biases (usflows_hip_internal.h)
        Ws.append(W)
        bs.append(b)
    Ws[0][:, ~geo["p_cols"][32 * kb_p0: 32 * (kb_p0 + c.nk_p)]] = 0
    t_rows = geo["t_cols"][32 * kb_t0: 32 * (kb_t0 + c.nk_t)]
    Ws[nh][~t_rows] = 0
    bs[nh][~t_rows] = 0
    p["W_eff"], p["W"], p["b"] = [], [], []
    ld_in, ld_hid, ld_out = Kin + 8 * (1 + c.idx % 2), 256 + 16, 256 + 8 * (1 + c.idx % 3)
    p["ld"] = (ld_in, ld_hid, ld_out)
    p["stride"] = [0, 0, 0]
    for l in range(nh + 1):
        ld = ld_in if l == 0 else (ld_out if l == nh else ld_hid)
        planes, flat, stride = _cw_image(Ws[l], npl, ld, 30 + l)
        p["W_eff"].append(plane_sum(planes))
        p["W"].append(flat)
        p["stride"][0 if l == 0 else (2 if l == nh else 1)] = stride
        p["b"].append(torch.cat([bs[l], nan_f32(8, 40 + l)]))
    if "ctx" in c.mode:
        wc, bc = torch.zeros(256), torch.zeros(256)
        wc[: c.hidden[0]] = torch.randn(c.hidden[0], generator=g)
        bc[: c.hidden[0]] = torch.randn(c.hidden[0], generator=g)
        p["w_ctx"], p["b_ctx"] = wc, bc
        n_ctx = M if c.ctx_stride == 1 else 1
        ctx = torch.randn(M, generator=g)[perm][:n_ctx] if c.ctx_stride == 1 else torch.randn(1, generator=g)
        p["ctx"] = torch.cat([ctx, nan_f32(EXTRA_ROWS, 50)])
    if c.mode == "side":
        # the fp32 values of the transformed blocks beside the planes; what z's transformed-only blocks hold is not read: NaN
        side_l = nan_f32(R * 32 * c.nk_t, 51).view(1, R, 32 * c.nk_t).clone()
        side_l[0, :M] = z_vals[:, 32 * kb_t0: 32 * (kb_t0 + c.nk_t)]
        p["S"] = torch.cat([nan_f32(GUARD // 4, 52), to_chunks(bits32(side_l)).view(torch.float32), nan_f32(GUARD // 4, 53)])
        zs = z_bits.clone()
        for kb in range(kb_t0, kb_t0 + c.nk_t):
            if not kb_p0 <= kb < kb_p0 + c.nk_p:
                zs[:, :, 32 * kb: 32 * kb + 32] = nan_bits16(npl * R * 32, npl, 54 + kb).view(npl, R, 32)
        p["z0_side_bits"] = zs
        p["z0_side"] = guarded(to_chunks(zs), npl, 21)
    if c.mode in ("hout", "hout_ctx", "gate"):
        p["hout0"] = [guarded(nan_bits16(3 * R * 256, 3, 60 + l), 3, 62 + l) for l in range(nh)]
    if c.mode == "gate":
        p["gate"], p["gate_eff"] = [], []
        for l in range(nh):
            hv = torch.randn(M, 256, generator=g)[perm]
            hv = torch.where(torch.rand(M, 256, generator=g)[perm] < 0.1, torch.zeros(()), hv).to(torch.bfloat16)
            gb = nan_bits16(3 * R * 256, 3, 70 + l).view(3, R, 256).clone()
            gb[0, :M] = bits16(hv)                      # only plane 0 is read; planes 1, 2 and the rows >= M stay NaN
            p["gate"].append(guarded(to_chunks(gb), 3, 72 + l))
            p["gate_eff"].append(hv.float())
    r64, r32 = coupling_forward(c, p, torch.float64), coupling_forward(c, p, torch.float32)
    p["ref64"], p["ref32"] = r64, r32
    tc = t_rows
    p["scale"], p["err32"], p["bound"] = _rel_bound(r64["t"][:, tc], r32["t"][:, tc], 2e-6)
    p["h_bounds"] = [_rel_bound(a, b, 2e-6) for a, b in zip(r64["hidden"], r32["hidden"])]
    return p


def coupling_inputs(c):
    names = [f"W{l}" for l in range(c.nh + 1)] + [f"b{l}" for l in range(c.nh + 1)]
    if "ctx" in c.mode:
        names += ["ctx", "w_ctx", "b_ctx"]
    if c.mode == "side":
        names += ["S"]
    if c.mode == "gate":
        names += [f"gate{l}" for l in range(c.nh)]
    return names


def coupling_buffers(c, p=None, side_form=True):
    """{name: CPU tensor} of everything a launch is handed; side_form = False: a "side" case as its plain twin (z holds the planes)"""
    p = p or coupling_prepared(c)
    b = {"z": (p["z0_side"] if c.mode == "side" and side_form else p["z0"]).clone()}
    for l in range(c.nh + 1):
        b[f"W{l}"], b[f"b{l}"] = p["W"][l], p["b"][l]
    if "ctx" in c.mode:
        b["ctx"], b["w_ctx"], b["b_ctx"] = p["ctx"], p["w_ctx"], p["b_ctx"]
    if c.mode == "side" and side_form:
        b["S"] = p["S"]
    if "hout0" in p:
        for l in range(c.nh):
            b[f"hout{l}"] = p["hout0"][l].clone()
    if c.mode == "gate":
        for l in range(c.nh):
            b[f"gate{l}"] = p["gate"][l]
    return b


def coupling_descriptor(c, ptr, desc_type, p=None, mode=None):
    """(usf_coupling_planes_desc, entry point, extra arguments); ptr(name): the address of buffer `name` as the launch must see it.
    mode: overrides the case's (the plain twin of a side / hout case)"""
    p = p or coupling_prepared(c)
    mode = mode or c.mode
    geo = coupling_geometry(c)
    d = desc_type()
    d.z, d.z_nkb, d.M = ptr("z"), geo["z_nkb"], c.M
    d.kb_p0, d.nk_p, d.kb_t0, d.nk_t = geo["kb_p0"], c.nk_p, geo["kb_t0"], c.nk_t
    d.n_hidden, d.hidden_padded = c.nh, 256
    d.W_in, d.ldw_in, d.w_in_plane, d.b_in = ptr("W0"), p["ld"][0], p["stride"][0], ptr("b0")
    for l in range(1, c.nh):
        d.W_hid[l - 1], d.b_hid[l - 1] = ptr(f"W{l}"), ptr(f"b{l}")
    d.ldw_hid, d.w_hid_plane = p["ld"][1], p["stride"][1]
    d.W_out, d.ldw_out, d.w_out_plane, d.b_out = ptr(f"W{c.nh}"), p["ld"][2], p["stride"][2], ptr(f"b{c.nh}")
    d.sign, d.slope, d.act, d.format, d.range_flag = c.sign, c.slope, c.act, fmt_of(c.npl), ptr("flag")
    if mode in ("hout", "hout_ctx", "gate"):
        for l in range(c.nh):
            d.hidden_out[l] = ptr(f"hout{l}")
    if mode == "gate":
        for l in range(c.nh):
            d.gate[l] = ptr(f"gate{l}")
    if "ctx" in mode:
        return d, "usf_coupling_planes_ctx", (ptr("ctx"), c.ctx_stride, ptr("w_ctx"), ptr("b_ctx"))
    if mode == "side":
        return d, "usf_coupling_planes_side", (ptr("S"), c.nk_t)
    return d, "usf_coupling_planes", ()


def coupling_as_launch(c, out, p=None, pad_rows=float("nan")):
    """the buffers as a launch that computes out = dict(t, hidden) would leave them: dict(z, hout0.., flag)"""
    p = p or coupling_prepared(c)
    geo = coupling_geometry(c)
    M, npl, R = c.M, c.npl, ceil_to(c.M, 16)
    bits = (p["z0_side_bits"] if c.mode == "side" else p["z0_bits"]).clone()
    t = out["t"].to(torch.float32)
    for nt in range(c.nk_t):
        sl = slice(32 * (geo["kb_t0"] + nt), 32 * (geo["kb_t0"] + nt) + 32)
        bits[:, :M, sl] = bits16(split_planes(t[:, 32 * nt: 32 * nt + 32].contiguous(), npl))
        if "ctx" not in c.mode:
            bits[:, M:, sl] = bits16(split_planes(torch.full((R - M, 32), pad_rows), npl))
    got = dict(z=guarded(to_chunks(bits), npl, 21), flag=0)
    if "hout0" in p:
        for l in range(c.nh):
            hb = torch.zeros(3, R, 256, dtype=torch.int16)
            hb[:, :M] = bits16(split_planes(out["hidden"][l].to(torch.float32).contiguous(), 3))
            hb[:, M:] = bits16(split_planes(torch.full((R - M, 256), pad_rows), 3))
            h0 = p["hout0"][l].clone()
            h0[GUARD // 2: h0.numel() - GUARD // 2] = to_chunks(hb)
            got[f"hout{l}"] = h0
    return got


def coupling_check(c, got, p=None):
    """(violations, figures) of dict(z, hout*, flag): every row < M of the transformed features within the bound of fp64, every
    other byte of z accounted for"""
    p = p or coupling_prepared(c)
    geo = coupling_geometry(c)
    M, npl, R = c.M, c.npl, ceil_to(c.M, 16)
    bad = []
    fig = dict(err=0.0, err32=p["err32"], bound=p["bound"])
    if int(got.get("flag", 0)) != 0:
        bad.append("range_flag raised")
    z, z0 = got["z"], (p["z0_side"] if c.mode == "side" else p["z0"])
    z0_bits = p["z0_side_bits"] if c.mode == "side" else p["z0_bits"]
    if z.shape != z0.shape:
        return [f"z has shape {tuple(z.shape)}"], fig
    g = GUARD // 2
    if not torch.equal(z[:g], z0[:g]) or not torch.equal(z[-g:], z0[-g:]):
        bad.append("z: a guard changed")
    bits = from_chunks(unguarded(z), npl, R // 16, geo["z_nkb"])
    t_blocks = torch.zeros(32 * geo["z_nkb"], dtype=torch.bool)
    t_blocks[32 * geo["kb_t0"]: 32 * (geo["kb_t0"] + c.nk_t)] = True
    # blocks the layer does not transform: conditioning-only blocks, the gap, the unused blocks -- every row, bit for bit
    if not torch.equal(bits[:, :, ~t_blocks], z0_bits[:, :, ~t_blocks]):
        bad.append(f"z: {int((bits[:, :, ~t_blocks] != z0_bits[:, :, ~t_blocks]).sum())} elements outside the transformed blocks changed")
    # the other set's features of the shared block: rewritten unchanged
    other = t_blocks & ~geo["t_cols"]
    # (as VALUES: two fp16 planes split again from their own sum may round a tie the other way; bf16x3 planes come back bit for bit)
    if other.any():
        now, was = (plane_sum(b[:, :M, other].contiguous().view(plane_dtype(npl))) for b in (bits, p["z0_bits"]))
        if not torch.equal(bits32(now), bits32(was)) or (npl == 3 and not torch.equal(bits[:, :M, other], p["z0_bits"][:, :M, other])):
            bad.append("z: conditioning features of the shared block changed")
    # rows >= M of the transformed blocks: untouched by a context launch, still no finite value otherwise
    pad = bits[:, M:, t_blocks]
    if pad.numel():
        if "ctx" in c.mode:
            if not torch.equal(pad, z0_bits[:, M:, t_blocks]):
                bad.append("z: a context launch wrote rows >= M")
        elif torch.isfinite(plane_sum(pad.contiguous().view(plane_dtype(npl)))).any():
            bad.append("z: a finite value in the rows >= M of a transformed block")
    pl = bits[:, :M, geo["t_cols"]].contiguous().view(plane_dtype(npl))
    v = plane_sum(pl)
    tc = geo["t_cols"][32 * geo["kb_t0"]: 32 * (geo["kb_t0"] + c.nk_t)]
    ref = p["ref64"]["t"][:, tc]
    if torch.isnan(v).any():
        bad.append(f"z: NaN in {int(torch.isnan(v).sum())} transformed elements of the rows < M")
    err = _max_rel(v, ref, p["scale"])
    fig["err"] = err.max().item()
    if fig["err"] > p["bound"]:
        r, k = divmod(int(err.argmax()), v.shape[1])
        bad.append(f"z: error {fig['err']:.3e} above the bound {p['bound']:.3e} (err32 {p['err32']:.3e}) at row {r}, transformed feature {k}")
    if not torch.isnan(v).any() and not _same_split(v, pl):
        bad.append("z: the planes are not the split of their sum")
    if "hout0" in p:
        for l in range(c.nh):
            h, h0 = got[f"hout{l}"], p["hout0"][l]
            if not torch.equal(h[:g], h0[:g]) or not torch.equal(h[-g:], h0[-g:]):
                bad.append(f"hidden_out[{l}]: a guard changed")
            hb = from_chunks(unguarded(h), 3, R // 16, 8)[:, :M].contiguous().view(torch.bfloat16)
            hv = plane_sum(hb)
            scale, err32, bound = p["h_bounds"][l]
            e = _max_rel(hv, p["ref64"]["hidden"][l], scale).max().item()
            fig["err"] = max(fig["err"], e * p["bound"] / bound)
            if e > bound:
                bad.append(f"hidden_out[{l}]: error {e:.3e} above the bound {bound:.3e} (err32 {err32:.3e})")
            if not torch.isnan(hv).any() and not _same_split(hv, hb):
                bad.append(f"hidden_out[{l}]: the planes are not the exact three-way split of their sum")
            w = c.hidden[l]
            if w < 256 and not bool((hv[:, w:] == 0).all()):
                bad.append(f"hidden_out[{l}]: hidden padding is not zero")
    return bad, fig


# ---- rows of a result, for the row-permutation test -----------------------------------------------------------------------------------
def gemm_rows(c, got, p=None):
    """everything a launch wrote for the rows < M as integer tensors with the row as their second-to-last dimension"""
    p = p or gemm_prepared(c)
    M, R = c.M, ceil_to(c.M, 16)
    if c.form == "fp32":
        out = [bits32(got["C"][p["c_off"]: p["c_off"] + (M + EXTRA_ROWS) * p["ldc"]].view(-1, p["ldc"])[:M, : c.n_out])] if c.store else []
        if c.base:
            out.append(bits32(got["part"].view(-1, 8)[:M, : gemm_grid(c)[1]]))
        return out
    written = torch.zeros(32 * c.c_nkb, dtype=torch.bool)
    for kbo, (to_planes, _) in enumerate(gemm_blocks(c)):
        written[32 * (c.c_kb0 + kbo): 32 * (c.c_kb0 + kbo) + 32] = to_planes
    out = [from_chunks(unguarded(got["C"]), c.npl, R // 16, c.c_nkb)[:, :M][:, :, written]]
    if c.form == "side":
        out.append(bits32(from_chunks(unguarded_f32(got["S"]), 1, R // 16, c.side[1])[:, :M]))
    return out


def coupling_rows(c, got):
    M, R = c.M, ceil_to(c.M, 16)
    geo = coupling_geometry(c)
    used = geo["p_cols"] | geo["t_cols"]          # (the poisoned blocks keep their own NaNs, row by row)
    out = [from_chunks(unguarded(got["z"]), c.npl, R // 16, geo["z_nkb"])[:, :M][:, :, used]]
    out += [from_chunks(unguarded(got[f"hout{l}"]), 3, R // 16, 8)[:, :M] for l in range(c.nh) if f"hout{l}" in got]
    return out
