"""The planes coupling kernel's cheaper vector work (profiles/coupling_valu_diet.md) on a real MI355X, through the C ABI:
the max form of the leaky ReLU against the select form bit for bit (knob coupling_act_max), the same launches against the
fp64 formula -- the smallest shapes at which the 32-bit addressing can go wrong: a ragged last panel, a partial last block of
waves, a straddling block, the last output block, every plane -- and the 4 GiB check of the host wrapper."""
import ctypes
import functools

import pytest
import torch

import emulator

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FMT = {"bf16x3": 0, "f16x2": 1}
NKB, KB_P0, NK_P, KB_T0, NK_T = 3, 0, 2, 1, 2       # conditioning blocks [0, 2), transformed blocks [1, 3): block 1 straddles
N_COND = 48                                        # features 0..47 condition, 48..95 are transformed
WIDTHS = [200, 136]
SLOPES_MAX = [0.01, 0.0, 1.0]                      # 0 <= slope <= 1: the max form
SLOPES_SELECT = [1.5, -0.2]                        # every other slope: the select form whatever the knob says
DENORM = 1e-40                                     # a denormal of fp32


def _ext():
    from usflows_amd import _ext
    _ext.load()
    return _ext


class act_max:
    """knob coupling_act_max for the duration of a block; back to its default (1) afterwards"""

    def __init__(self, v):
        self.v = v

    def _set(self, v):
        ext = _ext()
        ext.check(ext.load().usf_set_tuning(b"coupling_act_max", int(v)), "usf_set_tuning")

    def __enter__(self):
        self._set(self.v)

    def __exit__(self, *exc):
        self._set(1)


def _view(buf, M, nkb, fmt=0):
    npl, dt = (2, torch.float16) if fmt == 1 else (3, torch.bfloat16)
    return buf.cpu().view(dt).view(-(-M // 16), nkb, npl, 64, 8)


def _weight_planes(W, fmt, neg_zero_rows=()):
    """[3, rows, K] bf16 / [2, rows, K] fp16 planes of W [rows, K] with the slot permutation on K (K % 32 == 0); the residual
    planes of neg_zero_rows (rows of exactly representable weights <= 0: residuals zero) carry -0 wherever they hold a zero, so
    that every product of such a row with +0 is -0"""
    K = W.shape[1]
    phys = torch.tensor([32 * (c // 32) + emulator._slot_feature(c % 32) for c in range(K)])
    Wp = W[:, phys]
    dt = torch.float16 if fmt == 1 else torch.bfloat16
    p1 = Wp.to(dt)
    r = Wp - p1.float()
    p2 = r.to(dt)
    planes = [p1, p2] if fmt == 1 else [p1, p2, (r - p2.float()).to(dt)]
    for row in neg_zero_rows:
        assert (p1[row] <= 0).all()
        p1[row] = torch.where(p1[row] == 0, torch.full_like(p1[row], -0.0), p1[row])
        for pl in planes[1:]:
            assert (pl[row] == 0).all()
            pl[row] = -0.0
    return torch.stack(planes).contiguous()


def _special_units(W, b):
    """rows 0..4 of a layer (W [h, k], b [h]): pre-activations that are exactly +0, -0 (where the layer's input row is all +0:
    a negative weight times +0 on a bias of -0), and positive / negative denormals"""
    W[0] = 0; b[0] = 0.0
    W[1] = -0.5; b[1] = -0.0
    W[2] = 0; b[2] = -DENORM
    W[3] = 0; b[3] = -1.4e-45
    W[4] = 0; b[4] = DENORM


@functools.lru_cache(maxsize=None)
def _case(M, nh, fmt):
    """inputs of one layer shape, built once: logical matrices for the formula and device images for the kernel"""
    ext = _ext()
    f = FMT[fmt]
    g = torch.Generator().manual_seed(1000 * M + 10 * nh + f)
    widths = WIDTHS[:nh]
    X = torch.randn(M, 32 * NKB, generator=g) * 2
    for r in (3, 16, M - 1):                                               # rows whose conditioning BLOCKS are all +0
        X[r, : 32 * (KB_P0 + NK_P)] = 0.0
    k_in = 32 * NK_P
    Ws, bs = [], []
    W0 = torch.randn(widths[0], k_in, generator=g) / 7.0
    b0 = torch.randn(widths[0], generator=g) * 0.1
    _special_units(W0, b0)
    W0[:, N_COND - 32 * KB_P0:] = 0                                        # zero weights on the transformed features
    Ws.append(W0); bs.append(b0)
    for j in range(1, nh):
        W = torch.randn(widths[j], widths[j - 1], generator=g) / widths[j - 1] ** 0.5
        b = torch.randn(widths[j], generator=g) * 0.1
        _special_units(W, b)
        Ws.append(W); bs.append(b)
    Wo = torch.randn(32 * NK_T, widths[-1], generator=g) / widths[-1] ** 0.5
    bo = torch.randn(32 * NK_T, generator=g) * 0.1
    dead = torch.arange(32 * KB_T0, 32 * (KB_T0 + NK_T)) < N_COND            # the conditioning features of the straddling block
    Wo[dead] = 0; bo[dead] = 0

    def pad(W, rows, cols):
        o = torch.zeros(rows, cols); o[: W.shape[0], : W.shape[1]] = W; return o

    def padv(b, n):
        o = torch.zeros(n); o[: b.numel()] = b; return o

    zbuf = torch.zeros(ext.planes_bytes(M, NKB, f), dtype=torch.uint8)
    emulator.planes_encode(_view(zbuf, M, NKB, f), X, 0)
    X = emulator.planes_decode(_view(zbuf, M, NKB, f), M)                  # what the buffer holds
    dev = dict(
        Wi=_weight_planes(pad(Ws[0], 256, k_in), f, neg_zero_rows=(1,)).to(DEV), b0=padv(bs[0], 256).to(DEV),
        Wh=[_weight_planes(pad(Ws[j], 256, 256), f, neg_zero_rows=(1,)).to(DEV) for j in range(1, nh)],
        bh=[padv(bs[j], 256).to(DEV) for j in range(1, nh)],
        Wo=_weight_planes(pad(Wo, 32 * NK_T, 256), f).to(DEV), bo=bo.to(DEV))
    assert torch.equal(dev["b0"][1].cpu().view(torch.int32), torch.tensor(-0.0).view(torch.int32))   # the -0 bias arrives as -0
    return dict(M=M, nh=nh, f=f, X=X, zbuf=zbuf, Ws=Ws, bs=bs, Wo=Wo, bo=bo, dev=dev)


def _desc(c, zd, flag, sign, slope):
    ext = _ext()
    d, v = ext.CouplingPlanesDesc(), c["dev"]
    d.z, d.z_nkb, d.M = zd.data_ptr(), NKB, c["M"]
    d.kb_p0, d.nk_p, d.kb_t0, d.nk_t = KB_P0, NK_P, KB_T0, NK_T
    d.n_hidden, d.hidden_padded = c["nh"], 256
    d.W_in, d.ldw_in, d.w_in_plane = v["Wi"].data_ptr(), v["Wi"].shape[2], v["Wi"].shape[1] * v["Wi"].shape[2]
    d.b_in = v["b0"].data_ptr()
    for j, (Wh, bh) in enumerate(zip(v["Wh"], v["bh"])):
        d.W_hid[j], d.b_hid[j] = Wh.data_ptr(), bh.data_ptr()
        d.ldw_hid, d.w_hid_plane = Wh.shape[2], Wh.shape[1] * Wh.shape[2]
    d.W_out, d.ldw_out, d.w_out_plane = v["Wo"].data_ptr(), v["Wo"].shape[2], v["Wo"].shape[1] * v["Wo"].shape[2]
    d.b_out = v["bo"].data_ptr()
    d.sign, d.slope, d.act, d.format, d.range_flag = sign, slope, 1, c["f"], flag.data_ptr()
    return d


def _run(c, sign, slope, knob):
    """one launch on a fresh copy of the case's buffer: the bytes of z afterwards"""
    ext = _ext()
    zd = c["zbuf"].to(DEV)
    flag = torch.zeros(1, dtype=torch.int32, device=DEV)
    d = _desc(c, zd, flag, sign, slope)
    with act_max(knob):
        ext.check(ext.load().usf_coupling_planes(ctypes.byref(d), ext.current_stream(zd.device)), "usf_coupling_planes")
        torch.cuda.synchronize()
    assert int(flag.item()) == 0
    return zd.cpu()


def _formula(c, sign, slope, dt):
    X = c["X"]
    h = X[:, 32 * KB_P0: 32 * (KB_P0 + NK_P)].to(dt)
    for W, b in zip(c["Ws"], c["bs"]):
        h = torch.nn.functional.leaky_relu(h @ W.to(dt).t() + b.to(dt), slope)
    return X[:, 32 * KB_T0: 32 * (KB_T0 + NK_T)].to(dt) + sign * (h @ c["Wo"].to(dt).t() + c["bo"].to(dt))


CASES = [(M, nh, fmt) for M in (40, 200) for nh in (1, 2) for fmt in ("bf16x3", "f16x2")]


@pytest.mark.parametrize("M,nh,fmt", CASES)
def test_max_form_stores_the_select_forms_bytes(M, nh, fmt):
    """knob 1 (max(x, slope x) for 0 <= slope <= 1) against knob 0 (the select) on identical inputs, pre-activations of +0, -0
    and denormals among them: every stored byte of z is the same, both signs, every slope"""
    c = _case(M, nh, fmt)
    for sign in (1.0, -1.0):
        for slope in SLOPES_MAX + SLOPES_SELECT:
            new, old = _run(c, sign, slope, 1), _run(c, sign, slope, 0)
            assert torch.equal(new, old), (sign, slope, int((new != old).sum()))
            assert not torch.equal(new, c["zbuf"])                         # the launch did write


@pytest.mark.parametrize("M,nh,fmt", CASES)
def test_same_launches_against_the_fp64_formula(M, nh, fmt):
    """every row (the ragged last panel, the second block's waves), both output blocks, every plane against torch fp64 of the
    same layer at test_planes_gpu.py's tolerance; slopes outside [0, 1] under knob 1 show the select form taken (the max form
    of such a slope is another function)"""
    c = _case(M, nh, fmt)
    f = c["f"]
    rows = 16 * torch.arange(-(-M // 16)).view(-1, 1) + torch.arange(64).view(1, -1) % 16 < M       # [panel, line]: a real row
    for sign in (1.0, -1.0):
        for slope in SLOPES_MAX + SLOPES_SELECT:
            zb = _run(c, sign, slope, 1)
            got = emulator.planes_decode(_view(zb, M, NKB, f), M)
            r64, r32 = _formula(c, sign, slope, torch.float64), _formula(c, sign, slope, torch.float32)
            out = got[:, 32 * KB_T0: 32 * (KB_T0 + NK_T)].double()
            scale = r64.abs().max().item()
            err = (out - r64).abs().max(dim=0).values / scale             # per output feature
            err32 = (r32.double() - r64).abs().max().item() / scale
            tol = max(4 * err32, 2e-6)
            print(f"M {M} nh {nh} {fmt} sign {sign} slope {slope}: err {err.max().item():.3e} (fp32 formula {err32:.3e})")
            assert err.max().item() < tol, (sign, slope, err.max().item(), err32)
            last = slice(M - (M % 16 or 16), M)                            # the last panel's rows; the last output block
            assert ((out - r64)[last].abs().max().item() / scale) < tol and err[-32:].max().item() < tol
            # the conditioning-only block untouched, the conditioning features of the straddling block rewritten unchanged
            assert torch.equal(got[:, : N_COND], c["X"][:, : N_COND])
            if f == 0:
                # every plane, plane 2 included: what is stored is the exact three-way split of the value it sums to
                again = torch.zeros_like(zb)
                emulator.planes_encode(_view(again, M, NKB, f), got, 0)
                a, b = _view(zb, M, NKB, f).view(torch.int16), _view(again, M, NKB, f).view(torch.int16)
                for q in range(3):
                    assert torch.equal(a[:, :, q][rows.unsqueeze(1).expand(-1, NKB, -1)], b[:, :, q][rows.unsqueeze(1).expand(-1, NKB, -1)]), q


def test_a_geometry_of_4_gib_is_refused_before_any_launch():
    """z of 2^27 panels x 3 blocks (1.2 TB by its geometry): the error code, and nothing launched -- the pointers are not
    dereferenceable, a launch would fault"""
    ext = _ext()
    d = ext.CouplingPlanesDesc()
    fake = 1 << 20                                                         # 16-byte aligned, never read
    d.z, d.z_nkb, d.M = fake, NKB, 0x7fffffff
    d.kb_p0, d.nk_p, d.kb_t0, d.nk_t = KB_P0, NK_P, KB_T0, NK_T
    d.n_hidden, d.hidden_padded = 1, 256
    d.W_in, d.ldw_in, d.w_in_plane = fake, 64, 256 * 64
    d.b_in = fake
    d.W_out, d.ldw_out, d.w_out_plane = fake, 256, 64 * 256
    d.b_out = fake
    d.sign, d.slope, d.act, d.format, d.range_flag = 1.0, 0.01, 1, 0, 0
    torch.cuda.synchronize()
    rc = ext.load().usf_coupling_planes(ctypes.byref(d), ext.current_stream(torch.device(DEV)))
    assert rc == -3, rc
    assert "4 GiB" in ext.load().usf_last_error().decode()
    torch.cuda.synchronize()                                               # nothing ran: no fault to report
