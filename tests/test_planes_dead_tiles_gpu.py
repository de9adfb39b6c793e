"""Dead output tiles of the planes GEMM, on a real MI355X: a layer whose width is no multiple of the column tile ends in weight
rows that are zero, and usf_gemm_planes_bf16x3 looks for them on the device and leaves the products of an all-zero last 16-row
tile out (library knob planes_skip_dead, default 1; 0 = every tile runs in full).  Every case here launches the same descriptor
with the knob at 1 and at 0 and compares the outputs value for value (plane by plane, so that only +0 / -0 may differ), and
checks the knob = 1 output against the fp64 product within the bounds tests/test_planes_gpu.py uses for the same kernel.  The
fused coupling's panel order (knob coupling_descend) and the input pack's row kernel (knobs pack_wide, pack_rows) are held to
their other forms the same way."""
import ctypes
import math

import pytest
import torch

import emulator
from golden_util import load_case
from model_util import build_flow

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FMT = {"bf16x3": 0, "f16x2": 1}
M = 40                      # three row panels, the last one ragged


def _ext():
    from usflows_amd import _ext
    _ext.load()
    return _ext


class knobs:
    """library tuning knobs for the duration of a block; back to their defaults (1) afterwards"""

    def __init__(self, **kv):
        self.kv = kv

    def _set(self, name, v):
        ext = _ext()
        ext.check(ext.load().usf_set_tuning(name.encode(), int(v)), "usf_set_tuning")

    def __enter__(self):
        for k, v in self.kv.items():
            self._set(k, v)

    def __exit__(self, *exc):
        for k in self.kv:
            self._set(k, 1)


def _planes(buf, m, nkb, fmt=0):
    npl, dt = (2, torch.float16) if fmt == 1 else (3, torch.bfloat16)
    return buf.cpu().view(dt).view(-(-m // 16), nkb, npl, 64, 8)


def _same_values(b1, b0, m, nkb, fmt=0):
    """plane by plane, element by element: equal as numbers (+0 == -0), and nothing non-finite"""
    v1, v0 = _planes(b1, m, nkb, fmt).float(), _planes(b0, m, nkb, fmt).float()
    return bool(torch.isfinite(v1).all()) and torch.equal(v1, v0)


_PHYS = {}


def _phys(K):
    if K not in _PHYS:
        _PHYS[K] = torch.tensor([32 * (c // 32) + emulator._slot_feature(c % 32) for c in range(K)])
    return _PHYS[K]


def _weight_planes(W, fmt=0):
    """[3, rows, K] bf16 / [2, rows, K] fp16 planes of W [rows, K] with the slot permutation on K"""
    Wp = W[:, _phys(W.shape[1])]
    dt = torch.float16 if fmt == 1 else torch.bfloat16
    p1 = Wp.to(dt)
    r = Wp - p1.float()
    p2 = r.to(dt)
    if fmt == 1:
        return torch.stack([p1, p2]).contiguous()
    return torch.stack([p1, p2, (r - p2.float()).to(dt)]).contiguous()


def _encode(X, nkb, fmt=0):
    buf = torch.zeros(_ext().planes_bytes(X.shape[0], nkb, fmt), dtype=torch.uint8)
    emulator.planes_encode(_planes(buf, X.shape[0], nkb, fmt), X, 0)
    return buf


# ---------------------------------------------------------------------------------------------------------------------------------
# GEMM, planes output
# ---------------------------------------------------------------------------------------------------------------------------------
NK = 2
GEMM_CASES = {
    # name: (c_kbn, w_rows, zero rows (from, to), fmt, flags)
    "tn5_dead": (5, 160, (144, 160), "bf16x3", {}),
    "tn5_one_element_in_plane_2": (5, 160, (144, 160), "bf16x3", dict(poke=2)),
    "tn5_bias_in_the_dead_columns": (5, 160, (144, 160), "bf16x3", dict(dead_bias=True)),
    "tn5_two_column_tiles": (10, 320, (304, 320), "bf16x3", {}),
    "tn5_residual_and_leaky_relu": (5, 160, (144, 160), "bf16x3", dict(residual=True, act=True)),
    "tn4_rows_not_in_memory": (6, 192, (176, 192), "bf16x3", {}),
    "tn4_dead_beyond_the_output": (7, 256, (224, 256), "bf16x3", {}),
    "tn4_dead": (8, 256, (240, 256), "bf16x3", {}),
    "tn5_dead_f16x2": (5, 160, (144, 160), "f16x2", {}),
}


def _gemm_case(name):
    c_kbn, w_rows, (z0, z1), fmt, flags = GEMM_CASES[name]
    f = FMT[fmt]
    g = torch.Generator().manual_seed(sum(map(ord, name)))
    K = 32 * NK
    X = torch.randn(M, K, generator=g) * 3
    W = torch.randn(w_rows, K, generator=g) / math.sqrt(K)
    W[z0:z1] = 0
    bias = torch.randn(w_rows, generator=g)
    if not flags.get("dead_bias"):
        bias[z0:z1] = 0
    Wp = _weight_planes(W, f)
    poke = None
    if "poke" in flags:
        # one element of ONE plane, in the last K block of the last row: the rows are no longer zero.  (The third weight plane
        # meets the activations' first plane only: the element adds 1.0 * bf16(x) to its output.)
        assert flags["poke"] == 2
        Wp[2, w_rows - 1, K - 5] = 1.0
        poke = (w_rows - 1, int(_phys(K)[K - 5]))
    R = torch.randn(M, 32 * c_kbn, generator=g) * 2
    return dict(c_kbn=c_kbn, w_rows=w_rows, fmt=f, flags=flags, X=X, W=W, bias=bias, Wp=Wp, R=R, K=K, poke=poke)


def _run_gemm(c, knob, X=None):
    ext = _ext()
    f, flags, c_kbn = c["fmt"], c["flags"], c["c_kbn"]
    A = _encode(c["X"] if X is None else X, NK, f).to(DEV)
    Cd = _encode(c["R"], c_kbn, f).to(DEV)
    flag = torch.zeros(1, dtype=torch.int32, device=DEV)
    with knobs(planes_skip_dead=knob):
        ext.gemm_planes(A, c["Wp"].to(DEV), M=M, a_nkb=NK, nk=NK, bias=c["bias"].to(DEV), C_planes=Cd, c_nkb=c_kbn, c_kbn=c_kbn,
                        residual=Cd if flags.get("residual") else None, res_sign=-1.0, act=1 if flags.get("act") else 0,
                        slope=0.01, fmt=f, range_flag=flag)
        torch.cuda.synchronize()
    return Cd, int(flag.item())


@pytest.mark.parametrize("name", list(GEMM_CASES))
def test_gemm_planes_dead_tile_skip_changes_no_value(name):
    c = _gemm_case(name)
    f, flags, c_kbn, K = c["fmt"], c["flags"], c["c_kbn"], c["K"]
    got1, flag1 = _run_gemm(c, 1)
    got0, flag0 = _run_gemm(c, 0)
    assert _same_values(got1, got0, M, c_kbn, f), name
    assert flag1 == 0 and flag0 == 0
    out = emulator.planes_decode(_planes(got1, M, c_kbn, f), M).double()
    Rb = emulator.planes_decode(_planes(_encode(c["R"], c_kbn, f), M, c_kbn, f), M)       # what the buffer held
    Xb = emulator.planes_decode(_planes(_encode(c["X"], NK, f), M, NK, f), M)               # (fp16x2: X rounded to 22 bits)
    n = 32 * c_kbn

    def ref(dt):
        v = Xb.to(dt) @ c["W"][:n].to(dt).t() + c["bias"][:n].to(dt)
        if c["poke"] is not None:
            v[:, c["poke"][0]] += Xb[:, c["poke"][1]].to(torch.bfloat16).to(dt)
        if flags.get("act"):
            v = torch.nn.functional.leaky_relu(v, 0.01)
        return Rb.to(dt) - v if flags.get("residual") else v

    r64, r32 = ref(torch.float64), ref(torch.float32)
    scale = r64.abs().max().item()
    err = (out - r64).abs().max().item() / scale
    err32 = (r32.double() - r64).abs().max().item() / scale
    print(f"{name}: err {err:.3e} (fp32 reference {err32:.3e})")
    assert err < max(4 * err32, 6e-8 * math.sqrt(K)), (err, err32)          # tests/test_planes_gpu.py::test_gemm_planes_parity
    assert err < 1e-5
    if flags.get("dead_bias"):
        # the dead slots hold the (exactly split) bias
        assert torch.equal(out[:, 144:160].float(), c["bias"][144:160].expand(M, 16))


def test_gemm_planes_dead_tile_is_really_left_out():
    """Not part of the contract, used as a probe: a row with a non-finite activation turns its dead slots into NaN on the full
    path (0 * inf) and leaves the bias where the dead tile's products are left out -- so the knob = 1 launch of the all-zero case
    shows the skip taken, and the launches whose rows are not zero / not in memory show it not taken."""
    for name, taken, cols in (("tn5_bias_in_the_dead_columns", True, (144, 160)), ("tn5_one_element_in_plane_2", False, (144, 160)),
                              ("tn4_rows_not_in_memory", False, (176, 192)), ("tn4_dead", True, (240, 256)),
                              ("tn5_two_column_tiles", True, (304, 320)), ("tn5_dead_f16x2", True, (144, 160))):
        c = _gemm_case(name)
        X = c["X"].clone()
        X[17, 3] = float("inf")
        got1, _ = _run_gemm(c, 1, X)
        got0, _ = _run_gemm(c, 0, X)
        o1 = emulator.planes_decode(_planes(got1, M, c["c_kbn"], c["fmt"]), M)[17, cols[0]: cols[1]]
        o0 = emulator.planes_decode(_planes(got0, M, c["c_kbn"], c["fmt"]), M)[17, cols[0]: cols[1]]
        assert torch.isnan(o0).all(), name
        assert bool(torch.isfinite(o1).all()) == taken, name
        if name == "tn5_two_column_tiles":       # the first column tile's last feature tile is live: never skipped
            first = emulator.planes_decode(_planes(got1, M, c["c_kbn"], c["fmt"]), M)[17, 144:160]
            assert not torch.isfinite(first).any()


def test_gemm_planes_output_rows_must_be_in_memory():
    """w_rows = 32 c_kbn - 16 is refused by the entry point (w_rows >= 32 c_kbn is its contract); rows that are not in memory occur
    only beyond the stored blocks (case tn4_rows_not_in_memory above: the second column tile's rows 192..255, read clamped)"""
    ext = _ext()
    A = torch.zeros(ext.planes_bytes(M, NK), dtype=torch.uint8, device=DEV)
    W = torch.zeros(3, 144, 64, dtype=torch.bfloat16, device=DEV)
    Cd = torch.zeros(ext.planes_bytes(M, 5), dtype=torch.uint8, device=DEV)
    with pytest.raises(RuntimeError):
        ext.gemm_planes(A, W, M=M, a_nkb=NK, nk=NK, C_planes=Cd, c_nkb=5, c_kbn=5)


# ---------------------------------------------------------------------------------------------------------------------------------
# GEMM, fp32 output with the base density in the epilogue
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("store_rows", [True, False])
@pytest.mark.parametrize("base", ["laplace", "normal"])
def test_gemm_planes_f32_output_with_base_part(base, store_rows):
    ext = _ext()
    N, w_rows, K = 144, 160, 32 * NK
    g = torch.Generator().manual_seed(7 + (base == "normal"))
    X = torch.randn(M, K, generator=g) * 3
    W = torch.randn(w_rows, K, generator=g) / math.sqrt(K)
    W[N:] = 0
    bias = torch.randn(w_rows, generator=g); bias[N:] = 0
    loc, scale = torch.randn(N, generator=g) * 0.3, torch.rand(N, generator=g) + 0.5
    bid = ext.BASE_LAPLACE if base == "laplace" else ext.BASE_NORMAL
    stride = 160
    tab = torch.zeros(3 * stride, device=DEV)
    ext.base_tables(bid, loc.to(DEV), scale.to(DEV), N, tab, stride)
    A, Wp, bd = _encode(X, NK).to(DEV), _weight_planes(W).to(DEV), bias.to(DEV)

    def run(knob):
        C = torch.full((M, N), float("nan"), device=DEV)
        part = torch.full((M, 8), float("nan"), device=DEV)
        d = ext.GemmPlanesDesc()
        d.A, d.a_nkb, d.a_kb0, d.nk = A.data_ptr(), NK, 0, NK
        d.W_planes, d.ldw, d.w_plane_stride, d.w_rows = Wp.data_ptr(), K, w_rows * K, w_rows
        d.bias, d.C_f32, d.ldc, d.N, d.M = bd.data_ptr(), (C.data_ptr() if store_rows else None), N, N, M
        d.base_tab, d.base_tab_stride, d.base_part, d.base = tab.data_ptr(), stride, part.data_ptr(), bid
        with knobs(planes_skip_dead=knob):
            ext.check(ext.load().usf_gemm_planes_bf16x3(ctypes.byref(d), ext.current_stream(A.device)), "usf_gemm_planes_bf16x3")
            torch.cuda.synchronize()
        return C.cpu(), part.cpu()

    C1, p1 = run(1)
    C0, p0 = run(0)
    assert torch.equal(p1[:, 0], p0[:, 0]) and torch.isfinite(p1[:, 0]).all()
    z64 = X.double() @ W[:N].double().t() + bias[:N].double()
    d64 = (z64 - loc.double()) / scale.double()
    if base == "laplace":
        lp = (-d64.abs() - torch.log(2 * scale.double())).sum(1)
    else:
        lp = (-0.5 * d64 * d64 - torch.log(scale.double()) - 0.5 * math.log(2 * math.pi)).sum(1)
    assert ((p1[:, 0].double() - lp).abs() / lp.abs()).max().item() < 1e-5
    if store_rows:
        assert torch.equal(C1, C0)
        z32 = X @ W[:N].t() + bias[:N]
        sc = z64.abs().max().item()
        err, err32 = (C1.double() - z64).abs().max().item() / sc, (z32.double() - z64).abs().max().item() / sc
        assert err < max(4 * err32, 6e-8 * math.sqrt(K)) and err < 1e-5, (err, err32)


# ---------------------------------------------------------------------------------------------------------------------------------
# fused coupling
# ---------------------------------------------------------------------------------------------------------------------------------
def _coupling_case(nh, fmt, seed, m):
    """z of 3 blocks; conditioning blocks 0..1 (features 0..39), transformed blocks 1..2 (features 40..79) sharing block 1;
    hidden width 40 padded to 256; W_out's rows 48..63 (logical positions 80..95: padding) zero, b_out there NOT zero"""
    f = FMT[fmt]
    g = torch.Generator().manual_seed(seed)
    X = torch.randn(m, 96, generator=g) * 2
    W0 = torch.zeros(256, 64); W0[:40, :40] = torch.randn(40, 40, generator=g) / math.sqrt(40)
    b0 = torch.zeros(256); b0[:40] = torch.randn(40, generator=g) * 0.1
    Wh = torch.zeros(256, 256); Wh[:40, :40] = torch.randn(40, 40, generator=g) / math.sqrt(40)
    bh = torch.zeros(256); bh[:40] = torch.randn(40, generator=g) * 0.1
    Wo = torch.zeros(64, 256); Wo[8:48, :40] = torch.randn(40, 40, generator=g) / math.sqrt(40)
    bo = torch.zeros(64); bo[8:48] = torch.randn(40, generator=g) * 0.1
    bo[48:] = torch.randn(16, generator=g)
    return dict(nh=nh, fmt=f, m=m, X=X, W0=W0, b0=b0, Wh=Wh, bh=bh, Wo=Wo, bo=bo)


def _run_coupling(c, descend, hidden_out=False, ctx=None):
    ext = _ext()
    f, nh, m = c["fmt"], c["nh"], c["m"]
    zd = _encode(c["X"], 3, f).to(DEV)
    keep = []

    def dev(t):
        t = t.to(DEV); keep.append(t); return t

    d = ext.CouplingPlanesDesc()
    d.z, d.z_nkb, d.M = zd.data_ptr(), 3, m
    d.kb_p0, d.nk_p, d.kb_t0, d.nk_t = 0, 2, 1, 2
    d.n_hidden, d.hidden_padded = nh, 256
    Wi = dev(_weight_planes(c["W0"], f))
    d.W_in, d.ldw_in, d.w_in_plane, d.b_in = Wi.data_ptr(), 64, 256 * 64, dev(c["b0"]).data_ptr()
    if nh == 2:
        Wh = dev(_weight_planes(c["Wh"], f))
        d.W_hid[0], d.b_hid[0], d.ldw_hid, d.w_hid_plane = Wh.data_ptr(), dev(c["bh"]).data_ptr(), 256, 256 * 256
    Wo = dev(_weight_planes(c["Wo"], f))
    d.W_out, d.ldw_out, d.w_out_plane, d.b_out = Wo.data_ptr(), 256, 64 * 256, dev(c["bo"]).data_ptr()
    flag = torch.zeros(1, dtype=torch.int32, device=DEV)
    d.sign, d.slope, d.act, d.format, d.range_flag = -1.0, 0.01, 1, f, flag.data_ptr()
    hout = []
    if hidden_out:
        for l in range(nh):
            hout.append(torch.zeros(ext.planes_bytes(m, 8), dtype=torch.uint8, device=DEV))
            d.hidden_out[l] = hout[l].data_ptr()
    with knobs(coupling_descend=descend):
        if ctx is None:
            rc = ext.load().usf_coupling_planes(ctypes.byref(d), ext.current_stream(zd.device))
        else:
            cv, wc, bc = (dev(t) for t in ctx)
            rc = ext.load().usf_coupling_planes_ctx(ctypes.byref(d), cv.data_ptr(), 1, wc.data_ptr(), bc.data_ptr(),
                                                    ext.current_stream(zd.device))
        ext.check(rc, "usf_coupling_planes")
        torch.cuda.synchronize()
    return zd, hout, int(flag.item())


def _coupling_ref(c, dt, ctx=None):
    m = c["m"]
    Xb = emulator.planes_decode(_planes(_encode(c["X"], 3, c["fmt"]), m, 3, c["fmt"]), m)
    h = Xb[:, :64].to(dt) @ c["W0"].to(dt).t() + c["b0"].to(dt)
    if ctx is not None:
        h = h + ctx[2].to(dt) + ctx[0].to(dt)[:, None] * ctx[1].to(dt)
    h = torch.nn.functional.leaky_relu(h, 0.01)
    if c["nh"] == 2:
        h = torch.nn.functional.leaky_relu(h @ c["Wh"].to(dt).t() + c["bh"].to(dt), 0.01)
    return Xb, Xb[:, 32:96].to(dt) - (h @ c["Wo"].to(dt).t() + c["bo"].to(dt))


COUPLING_CASES = [
    # rows (40: one block; 250: two blocks, the last panel ragged; 1100: nine blocks), n_hidden, format, hidden_out (MODE 1), context
    (40, 1, "bf16x3", False, False), (250, 1, "bf16x3", False, False), (250, 2, "bf16x3", False, False),
    (1100, 2, "bf16x3", False, False), (250, 1, "bf16x3", True, False), (250, 2, "bf16x3", True, False),
    (250, 1, "f16x2", False, False), (250, 2, "f16x2", False, False),
    (250, 2, "bf16x3", False, True), (250, 2, "bf16x3", True, True),
]


@pytest.mark.parametrize("m,nh,fmt,hidden_out,with_ctx", COUPLING_CASES)
def test_coupling_planes_panel_order_changes_no_byte(m, nh, fmt, hidden_out, with_ctx):
    """blocks that take the panels from the last one down (knob coupling_descend = 1, the default) write what ascending blocks write"""
    c = _coupling_case(nh, fmt, seed=100 + nh, m=m)
    ctx = None
    if with_ctx:
        g = torch.Generator().manual_seed(5)
        wc, bc = torch.zeros(256), torch.zeros(256)
        wc[:40], bc[:40] = torch.randn(40, generator=g) * 0.3, torch.randn(40, generator=g) * 0.1
        ctx = (torch.randn(m, generator=g), wc, bc)
    z1, h1, flag1 = _run_coupling(c, 1, hidden_out, ctx)
    z0, h0, flag0 = _run_coupling(c, 0, hidden_out, ctx)
    assert torch.equal(z1, z0)
    assert flag1 == 0 and flag0 == 0
    for a, b in zip(h1, h0):
        assert torch.equal(a, b)
    got = emulator.planes_decode(_planes(z1, m, 3, c["fmt"]), m)
    Xb, r64 = _coupling_ref(c, torch.float64, ctx)
    _, r32 = _coupling_ref(c, torch.float32, ctx)
    scale = r64.abs().max().item()
    err = (got[:, 32:96].double() - r64).abs().max().item() / scale
    err32 = (r32.double() - r64).abs().max().item() / scale
    print(f"m {m} nh {nh} {fmt} hidden_out {hidden_out} ctx {with_ctx}: err {err:.3e} (fp32 reference {err32:.3e})")
    assert err < max(4 * err32, 2e-6), (err, err32)          # tests/test_planes_gpu.py::test_coupling_planes_kernel_vs_reference_arithmetic
    assert torch.equal(got[:, :32], Xb[:, :32])              # the conditioning-only block is untouched
    assert torch.equal(got[:, 32:40], Xb[:, 32:40])          # the other set's features of the shared block: rewritten unchanged


# ---------------------------------------------------------------------------------------------------------------------------------
# input pack
# ---------------------------------------------------------------------------------------------------------------------------------
def _pack_index(kind, D, nkb):
    L = 32 * nkb
    idx = torch.full((L,), -1, dtype=torch.int32)
    if kind == "contiguous":
        idx[:D] = torch.arange(D, dtype=torch.int32)
    elif kind == "checkerboard":          # even columns first, then the odd ones: monotone inside each segment
        cols = torch.cat([torch.arange(0, D, 2), torch.arange(1, D, 2)]).to(torch.int32)
        idx[:D] = cols
    else:                                 # holes: -1 entries between the live ones, the live ones shuffled
        g = torch.Generator().manual_seed(D)
        n = min(D, L - 5)
        pos = torch.randperm(L, generator=g)[:n]
        idx[pos] = torch.randperm(D, generator=g)[:n].to(torch.int32)
    return idx


@pytest.mark.parametrize("pre", [False, True])
@pytest.mark.parametrize("fmt", ["bf16x3", "f16x2"])
@pytest.mark.parametrize("kind", ["checkerboard", "contiguous", "holes"])
@pytest.mark.parametrize("D", [33, 784])
def test_pack_planes_rows_kernel_writes_the_per_element_kernels_bytes(D, kind, fmt, pre):
    ext = _ext()
    f = FMT[fmt]
    nkb = -(-D // 32)
    g = torch.Generator().manual_seed(D + len(kind))
    x = (torch.randn(M, D, generator=g) * 5).to(DEV)
    idx = _pack_index(kind, D, nkb).to(DEV)
    pdiv = (torch.rand(32 * nkb, generator=g) + 0.5).to(DEV) if pre else None
    psub = torch.randn(32 * nkb, generator=g).to(DEV) if pre else None

    def run(rows, wide):
        buf = torch.full((ext.planes_bytes(M, nkb, f),), 0xAB, dtype=torch.uint8, device=DEV)
        flag = torch.zeros(1, dtype=torch.int32, device=DEV)
        with knobs(pack_rows=rows, pack_wide=wide):
            ext.pack_planes(x, buf, M=M, nkb=nkb, idx=idx, pre_div=pdiv, pre_sub=psub, fmt=f, range_flag=flag, src_cols=D)
            torch.cuda.synchronize()
        return buf, int(flag.item())

    b1, f1 = run(1, 1)          # whole rows through LDS, 512-thread blocks (the default)
    b2, f2 = run(1, 0)          # ... 256-thread blocks
    b0, f0 = run(0, 1)          # the per-element gather
    assert torch.equal(b1, b0) and torch.equal(b2, b0)
    assert f1 == 0 and f2 == 0 and f0 == 0


@pytest.mark.parametrize("wide", [1, 0])
def test_pack_planes_grad_form_still_matches_the_two_pass_form(wide):
    """GRAD (the head of the training backward) rides the row kernel: the planes of usf_base_logprob_grad_f32 + a plain pack"""
    ext = _ext()
    D, nkb = 33, 2
    g = torch.Generator().manual_seed(3)
    z = (torch.randn(M, D, generator=g) * 3).to(DEV)
    w, loc, scale = torch.randn(M, generator=g).to(DEV), torch.randn(D, generator=g).to(DEV), (torch.rand(D, generator=g) + 0.5).to(DEV)
    idx = _pack_index("checkerboard", D, nkb).to(DEV)
    b1 = torch.zeros(ext.planes_bytes(M, nkb), dtype=torch.uint8, device=DEV)
    b2 = torch.zeros_like(b1)
    with knobs(pack_wide=wide):
        ext.pack_planes(z, b1, M=M, nkb=nkb, idx=idx, src_cols=D, grad=(ext.BASE_LAPLACE, w, loc, scale))
        torch.cuda.synchronize()
    gbuf = torch.zeros(M, D, device=DEV)
    ext.base_logprob_grad(z, D, w, M, D, ext.BASE_LAPLACE, loc, scale, gbuf, D)
    with knobs(pack_rows=0):
        ext.pack_planes(gbuf, b2, M=M, nkb=nkb, idx=idx)
        torch.cuda.synchronize()
    assert torch.equal(b1, b2)


# ---------------------------------------------------------------------------------------------------------------------------------
# a whole flow
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["bf16x3", "f16x2"])
def test_flow_log_prob_is_bit_identical_with_all_knobs_off(fmt):
    spec, sd, a = load_case("synth_d64_k6_hh0_laplace")
    x = a["x"].to(DEV)
    out = []
    for v in (1, 0):
        with knobs(planes_skip_dead=v, coupling_descend=v, pack_wide=v, pack_rows=v):
            flow = build_flow(spec, sd, device=DEV)
            eng = flow.engine()
            eng.use_planes, eng.planes_min_rows, eng.gemm_mode = True, 0, fmt
            eng.use_fused_coupling, eng.fused_min_rows = True, 0
            with torch.no_grad():
                out.append(flow.log_prob(x).cpu())
            torch.cuda.synchronize()
            assert any(p.get("planes") for p in eng._plans.values()), "planes plan was not built"
    assert torch.equal(out[0], out[1])
    rel = ((out[0].double() - a["log_prob64"].double()).abs() / a["log_prob64"].double().abs()).max().item()
    assert rel < 1e-5
