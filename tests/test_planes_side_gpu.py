"""The fp32 hand-over of the transformed half from an affine GEMM to the fused coupling behind it (usf_gemm_planes_side /
usf_coupling_planes_side, include/usflows_hip_internal.h) on a real MI355X, through the C ABI.  A GEMM on planes followed by a
fused coupling, with the side buffer and without it, at the smallest shapes where the new addressing can go wrong: a ragged
last panel (100 rows), a partial last block of waves (16 * 8 * 2 + 16 rows), a block that holds conditioning and transformed
features at either end of the transformed range (D = 72), no such block (D = 64), a transformed range that crosses a column
block of 4 and of 5 blocks (D = 200), both plane formats, both signs.
  (a) the planes buffer behind the coupling is the same, byte for byte;
  (b) it agrees with the fp64 formula within tests/test_coupling_planes_valu_gpu.py's bound;
  (c) the bytes around the side buffer, around the planes buffer and in the planes blocks the GEMM no longer writes are
      untouched, and those blocks hold NaN patterns on entry: nothing depends on them;
  (d) the refusals of the two entry points, in front of any launch."""
import ctypes
import functools

import pytest
import torch

import emulator

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FMT = {"bf16x3": 0, "f16x2": 1}
GUARD = 4096
WIDTHS = [200, 136]
# nkb blocks per panel; logical positions [lo, hi) of the conditioning (p) and transformed (t) features; tn: forced column-block width
GEOS = {
    "d72": dict(nkb=3, p=(0, 36), t=(36, 72), tn=0),             # block 1 straddles: the FIRST block of the transformed range
    "d72_t_first": dict(nkb=3, p=(36, 72), t=(0, 36), tn=0),     # the masks alternate: block 1 straddles as the LAST block of the range
    "d64": dict(nkb=2, p=(0, 32), t=(32, 64), tn=0),             # no straddling block
    "d200_tn4": dict(nkb=7, p=(0, 100), t=(100, 200), tn=4),     # blocks 3..6 of column blocks [0, 4) [4, 8)
    "d200_tn5": dict(nkb=7, p=(0, 100), t=(100, 200), tn=5),     # ... of [0, 5) [5, 10)
}
ROWS = [100, 16 * 8 * 2 + 16]


def _ext():
    from usflows_amd import _ext
    _ext.load()
    return _ext


class planes_tn:
    """knob planes_tn (the GEMM's column-block width; 0 = the one that pads less) for the duration of a block"""

    def __init__(self, v):
        self.v = v

    def _set(self, v):
        ext = _ext()
        ext.check(ext.load().usf_set_tuning(b"planes_tn", int(v)), "usf_set_tuning")

    def __enter__(self):
        self._set(self.v)

    def __exit__(self, *exc):
        self._set(0)


def _view(buf, M, nkb, f):
    npl, dt = (2, torch.float16) if f == 1 else (3, torch.bfloat16)
    return buf.view(dt).view(-(-M // 16), nkb, npl, 64, 8)


def _weight_planes(W, f):
    """[NPL, rows, K] planes of W [rows, K] with the slot permutation on K (K % 32 == 0)"""
    K = W.shape[1]
    phys = torch.tensor([32 * (c // 32) + emulator._slot_feature(c % 32) for c in range(K)])
    Wp = W[:, phys]
    dt = torch.float16 if f == 1 else torch.bfloat16
    p1 = Wp.to(dt)
    r = Wp - p1.float()
    p2 = r.to(dt)
    planes = [p1, p2] if f == 1 else [p1, p2, (r - p2.float()).to(dt)]
    return torch.stack(planes).contiguous()


def _blocks(lo, hi):
    return lo // 32, -(-hi // 32) - lo // 32


@functools.lru_cache(maxsize=None)
def _case(geo, M, nh, fmt):
    """inputs of one (geometry, rows, format), built once: logical matrices for the formula, device images for the kernels"""
    ext, G, f = _ext(), GEOS[geo], FMT[fmt]
    nkb = G["nkb"]
    L = 32 * nkb
    D = max(G["p"][1], G["t"][1])
    g = torch.Generator().manual_seed(7919 * M + 31 * len(geo) + 3 * nkb + f)
    X = torch.randn(M, L, generator=g)
    X[:, D:] = 0
    A = torch.zeros(ext.planes_bytes(M, nkb, f), dtype=torch.uint8)
    emulator.planes_encode(_view(A, M, nkb, f), X, 0)
    X = emulator.planes_decode(_view(A, M, nkb, f), M)                     # what the buffer holds
    Wa = torch.randn(L, L, generator=g) / L ** 0.5
    ba = torch.randn(L, generator=g) * 0.3
    Wa[D:] = 0; Wa[:, D:] = 0; ba[D:] = 0
    (kb_p0, nk_p), (kb_t0, nk_t) = _blocks(*G["p"]), _blocks(*G["t"])
    pos_p, pos_t = torch.arange(32 * kb_p0, 32 * (kb_p0 + nk_p)), torch.arange(32 * kb_t0, 32 * (kb_t0 + nk_t))
    in_p, in_t = (pos_p >= G["p"][0]) & (pos_p < G["p"][1]), (pos_t >= G["t"][0]) & (pos_t < G["t"][1])
    widths = WIDTHS[:nh]
    Ws, bs = [], []
    W0 = torch.randn(widths[0], 32 * nk_p, generator=g) / 7.0
    W0[:, ~in_p] = 0                                                       # zero weights on everything but the conditioning features
    Ws.append(W0); bs.append(torch.randn(widths[0], generator=g) * 0.1)
    for j in range(1, nh):
        Ws.append(torch.randn(widths[j], widths[j - 1], generator=g) / widths[j - 1] ** 0.5)
        bs.append(torch.randn(widths[j], generator=g) * 0.1)
    Wo = torch.randn(32 * nk_t, widths[-1], generator=g) / widths[-1] ** 0.5
    bo = torch.randn(32 * nk_t, generator=g) * 0.1
    Wo[~in_t] = 0; bo[~in_t] = 0                                           # the other features of the range are rewritten unchanged

    def pad(W, rows, cols):
        o = torch.zeros(rows, cols); o[: W.shape[0], : W.shape[1]] = W; return o

    def padv(b, n):
        o = torch.zeros(n); o[: b.numel()] = b; return o

    dev = dict(A=A.to(DEV), Wa=_weight_planes(Wa, f).to(DEV), ba=ba.to(DEV),
               Wi=_weight_planes(pad(Ws[0], 256, 32 * nk_p), f).to(DEV), b0=padv(bs[0], 256).to(DEV),
               Wh=[_weight_planes(pad(Ws[j], 256, 256), f).to(DEV) for j in range(1, nh)],
               bh=[padv(bs[j], 256).to(DEV) for j in range(1, nh)],
               Wo=_weight_planes(pad(Wo, 32 * nk_t, 256), f).to(DEV), bo=bo.to(DEV))
    t_only = [kb for kb in range(kb_t0, kb_t0 + nk_t) if not (kb_p0 <= kb < kb_p0 + nk_p)]
    both = [kb for kb in range(kb_t0, kb_t0 + nk_t) if kb_p0 <= kb < kb_p0 + nk_p]
    return dict(geo=geo, M=M, nh=nh, f=f, nkb=nkb, L=L, X=X, Wa=Wa, ba=ba, Ws=Ws, bs=bs, Wo=Wo, bo=bo, dev=dev, tn=G["tn"],
                kb_p0=kb_p0, nk_p=nk_p, kb_t0=kb_t0, nk_t=nk_t, pos_p=pos_p, pos_t=pos_t, t_only=t_only, both=both)


def _gemm_desc(c, Cd, flag):
    ext = _ext()
    d, v = ext.GemmPlanesDesc(), c["dev"]
    d.A, d.a_nkb, d.a_kb0, d.nk, d.M = v["A"].data_ptr(), c["nkb"], 0, c["nkb"], c["M"]
    d.W_planes, d.ldw, d.w_plane_stride, d.w_rows = v["Wa"].data_ptr(), c["L"], c["L"] * c["L"], c["L"]
    d.bias = v["ba"].data_ptr()
    d.C_planes, d.c_nkb, d.c_kb0, d.c_kbn = Cd.data_ptr() + GUARD, c["nkb"], 0, c["nkb"]
    d.res_sign, d.act, d.format, d.range_flag = 1.0, 0, c["f"], flag.data_ptr()
    return d


def _cpl_desc(c, Cd, flag, sign):
    ext = _ext()
    d, v = ext.CouplingPlanesDesc(), c["dev"]
    d.z, d.z_nkb, d.M = Cd.data_ptr() + GUARD, c["nkb"], c["M"]
    d.kb_p0, d.nk_p, d.kb_t0, d.nk_t = c["kb_p0"], c["nk_p"], c["kb_t0"], c["nk_t"]
    d.n_hidden, d.hidden_padded = c["nh"], 256
    d.W_in, d.ldw_in, d.w_in_plane = v["Wi"].data_ptr(), v["Wi"].shape[2], v["Wi"].shape[1] * v["Wi"].shape[2]
    d.b_in = v["b0"].data_ptr()
    for j, (Wh, bh) in enumerate(zip(v["Wh"], v["bh"])):
        d.W_hid[j], d.b_hid[j] = Wh.data_ptr(), bh.data_ptr()
        d.ldw_hid, d.w_hid_plane = Wh.shape[2], Wh.shape[1] * Wh.shape[2]
    d.W_out, d.ldw_out, d.w_out_plane = v["Wo"].data_ptr(), v["Wo"].shape[2], v["Wo"].shape[1] * v["Wo"].shape[2]
    d.b_out = v["bo"].data_ptr()
    d.sign, d.slope, d.act, d.format, d.range_flag = sign, 0.01, 1, c["f"], flag.data_ptr()
    return d


def _planes_buf(c, fill):
    n = _ext().planes_bytes(c["M"], c["nkb"], c["f"])
    return torch.full((GUARD + n + GUARD,), fill, dtype=torch.uint8, device=DEV), n


def _side_args(c):
    b0, nb = (c["both"][0], len(c["both"])) if c["both"] else (c["kb_t0"], 0)
    return c["kb_t0"], c["nk_t"], b0, nb


def _pair(c, sign, side):
    """GEMM, then coupling, on a planes buffer that holds 0xFF bytes (NaN in either format) on entry.  Returns the buffer behind
    the GEMM, behind the coupling and (side: the side buffer behind the GEMM), guards included, on the host"""
    ext = _ext()
    lib, st = ext.load(), ext.current_stream(torch.device(DEV))
    Cd, n = _planes_buf(c, 0xFF)
    flag = torch.zeros(1, dtype=torch.int32, device=DEV)
    g, k = _gemm_desc(c, Cd, flag), _cpl_desc(c, Cd, flag, sign)
    with planes_tn(c["tn"]):
        if side:
            ns = -(-c["M"] // 16) * c["nk_t"] * 2048
            Sd = torch.full((GUARD + ns + GUARD,), 0xA5, dtype=torch.uint8, device=DEV)
            ext.check(lib.usf_gemm_planes_side(ctypes.byref(g), Sd.data_ptr() + GUARD, *_side_args(c), st), "usf_gemm_planes_side")
            after_gemm, side_buf = Cd.cpu(), Sd.cpu()
            ext.check(lib.usf_coupling_planes_side(ctypes.byref(k), Sd.data_ptr() + GUARD, c["nk_t"], st), "usf_coupling_planes_side")
            torch.cuda.synchronize()
            assert torch.equal(Sd.cpu(), side_buf)                         # the coupling only reads it
        else:
            ext.check(lib.usf_gemm_planes_bf16x3(ctypes.byref(g), st), "usf_gemm_planes_bf16x3")
            after_gemm, side_buf = Cd.cpu(), None
            ext.check(lib.usf_coupling_planes(ctypes.byref(k), st), "usf_coupling_planes")
            torch.cuda.synchronize()
    assert int(flag.item()) == 0
    return after_gemm, Cd.cpu(), side_buf


@functools.lru_cache(maxsize=None)
def _plain(geo, M, nh, fmt, sign):
    """the reference launches (no side buffer) of a case, run once and shared"""
    return _pair(_case(geo, M, nh, fmt), sign, False)


def _formula(c, sign, dt):
    Z = c["X"].to(dt) @ c["Wa"].to(dt).t() + c["ba"].to(dt)
    h = Z[:, c["pos_p"]]
    for W, b in zip(c["Ws"], c["bs"]):
        h = torch.nn.functional.leaky_relu(h @ W.to(dt).t() + b.to(dt), 0.01)
    out = Z.clone()
    out[:, c["pos_t"]] = Z[:, c["pos_t"]] + sign * (h @ c["Wo"].to(dt).t() + c["bo"].to(dt))
    return out


CASES = [(geo, M, fmt) for geo in GEOS for M in ROWS for fmt in FMT]


@pytest.mark.parametrize("geo,M,fmt", CASES)
def test_side_buffer_pair_stores_the_plain_pairs_bytes(geo, M, fmt):
    """(a) and (c): GEMM + coupling with the side buffer against the same pair without it, both signs"""
    nh = 2 if M == ROWS[0] else 1
    c = _case(geo, M, nh, fmt)
    f, nkb, npan = c["f"], c["nkb"], -(-M // 16)
    for sign in (1.0, -1.0):
        g0, z0, _ = _plain(geo, M, nh, fmt, sign)
        g1, z1, s1 = _pair(c, sign, True)
        n = g0.numel() - 2 * GUARD
        # behind the GEMM: the guards and the blocks it no longer writes still hold the bytes they held, every other block is the
        # plain GEMM's
        assert bool((g1[:GUARD] == 0xFF).all()) and bool((g1[GUARD + n:] == 0xFF).all())
        v0, v1 = _view(g0[GUARD: GUARD + n], M, nkb, f).view(torch.int16), _view(g1[GUARD: GUARD + n], M, nkb, f).view(torch.int16)
        for kb in range(nkb):
            if kb in c["t_only"]:
                assert bool((v1[:, kb] == -1).all()), (sign, kb)
            else:
                assert torch.equal(v1[:, kb], v0[:, kb]), (sign, kb)
        assert bool((v0 != -1).any(dim=-1).all())                         # (the plain GEMM wrote every line of every block)
        # the side buffer: untouched guards, and in every chunk the fp32 values the plain GEMM's planes sum to -- the rows of the
        # last panel beyond M included
        ns = npan * c["nk_t"] * 2048
        assert bool((s1[:GUARD] == 0xA5).all()) and bool((s1[GUARD + ns:] == 0xA5).all())
        got = s1[GUARD: GUARD + ns].view(torch.float32).view(npan, c["nk_t"], 64, 8)
        pl = _view(g0[GUARD: GUARD + n], M, nkb, f)[:, c["kb_t0"]: c["kb_t0"] + c["nk_t"]]
        want = pl[:, :, 0].float() + pl[:, :, 1].float()
        if f == 0:
            want = want + pl[:, :, 2].float()
        assert torch.equal(got.view(torch.int32), want.view(torch.int32)), sign
        # behind the coupling: the whole buffer, guards included, byte for byte
        assert torch.equal(z1, z0), (sign, int((z1 != z0).sum()))
        assert not torch.equal(z1, g1)


@pytest.mark.parametrize("geo,M,fmt", CASES)
def test_side_buffer_pair_against_the_fp64_formula(geo, M, fmt):
    """(b): every row and every block behind the pair with the side buffer against torch fp64 of the two layers, at the bound of
    tests/test_coupling_planes_valu_gpu.py: four times the fp32 formula's own error, at least 2e-6 of the largest value"""
    nh = 2 if M == ROWS[0] else 1
    c = _case(geo, M, nh, fmt)
    for sign in (1.0, -1.0):
        _, z1, _ = _pair(c, sign, True)
        n = z1.numel() - 2 * GUARD
        got = emulator.planes_decode(_view(z1[GUARD: GUARD + n], M, c["nkb"], c["f"]), M).double()
        r64, r32 = _formula(c, sign, torch.float64), _formula(c, sign, torch.float32)
        scale = r64.abs().max().item()
        err = (got - r64).abs().max(dim=0).values / scale                  # per position of the buffer
        err32 = (r32.double() - r64).abs().max().item() / scale
        tol = max(4 * err32, 2e-6)
        print(f"{geo} M {M} nh {nh} {fmt} sign {sign}: err {err.max().item():.3e} (fp32 formula {err32:.3e}, bound {tol:.3e})")
        assert err.max().item() < tol, (sign, err.max().item(), err32)
        last = slice(M - (M % 16 or 16), M)                                # the last panel's rows; the last transformed block
        assert ((got - r64)[last].abs().max().item() / scale) < tol and err[c["pos_t"][-32:]].max().item() < tol


def test_refusals_come_before_any_launch():
    """(d): a misaligned side buffer, block ranges outside the output, a both range outside the side range, a residual, a block
    count that is not the layer's: the error codes, and nothing launched -- the buffers still hold their fill"""
    ext = _ext()
    lib, st = ext.load(), ext.current_stream(torch.device(DEV))
    c = _case("d72", 100, 1, "bf16x3")
    Cd, n = _planes_buf(c, 0xFF)
    Sd = torch.full((GUARD + 7 * 3 * 2048 + GUARD,), 0xA5, dtype=torch.uint8, device=DEV)
    flag = torch.zeros(1, dtype=torch.int32, device=DEV)
    side = Sd.data_ptr() + GUARD

    def gemm(side_ptr, *rng, residual=False):
        g = _gemm_desc(c, Cd, flag)
        if residual:
            g.residual = g.C_planes
        return lib.usf_gemm_planes_side(ctypes.byref(g), side_ptr, *rng, st), lib.usf_last_error()

    for args, kw, rc, msg in [((side + 8, 1, 2, 1, 1), {}, -2, b"16-byte aligned"), ((None, 1, 2, 1, 1), {}, -1, b"null side"),
                              ((side, 2, 2, 2, 0), {}, -2, b"bad block ranges"), ((side, 1, 0, 1, 0), {}, -2, b"bad block ranges"),
                              ((side, 1, 2, 0, 1), {}, -2, b"bad block ranges"), ((side, 1, 2, 2, 2), {}, -2, b"bad block ranges"),
                              ((side, 1, 2, 1, 1), dict(residual=True), -2, b"no residual")]:
        got, err = gemm(*args, **kw)
        assert got == rc and msg in err, (args, kw, got, err)
    k = _cpl_desc(c, Cd, flag, 1.0)
    for side_ptr, nkb, rc, msg in [(side + 4, 2, -2, b"16-byte aligned"), (None, 2, -1, b"null side"), (side, 3, -2, b"blocks per panel")]:
        got = lib.usf_coupling_planes_side(ctypes.byref(k), side_ptr, nkb, st)
        assert got == rc and msg in lib.usf_last_error(), (side_ptr, nkb, got, lib.usf_last_error())
    torch.cuda.synchronize()
    assert bool((Cd == 0xFF).all()) and bool((Sd == 0xA5).all())
