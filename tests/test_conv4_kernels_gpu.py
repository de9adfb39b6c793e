"""Every forward row of tests/conv4_cases.py launched once on the device, in both placements of the 4 x 4 kernel's zeros, and held
to the file's own fp64 statement on EVERY element, in the manner of tests/test_conv5_kernels_gpu.py (``Launch`` of
tests/test_conv_kernels_gpu.py builds the operands: NaN samples behind every input, sentinels in front of and behind y): the
probe's answer for this device, the per-element bound MARGIN * K32_4 * U * A next to the checker's max-norm rule, the same bits
from a second launch, batch (a) as a bit-exact prefix of batch (b); the mirrored entry point on flipped, transposed planes against
autograd's data gradient of the fp64 statement; the device plane split at ks = 4; usf_conv_wgrad_k4_f32 and the 16-tap
usf_conv_ctx_wgrad_f32 against fp64 at 2e-6 * max|ref| (the bound rule of tests/wide_wgrad_cases.py's tests)."""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import conv_kernel_cases as K  # noqa: E402
import conv4_cases as K4  # noqa: E402
from test_conv_kernels_gpu import Launch, _variant, DEV  # noqa: E402

pytestmark = pytest.mark.gpu
CASES = {c.name: c for c in K4.cases()}
BOUND = K.MARGIN * K4.K32_4


def _ext():
    from usflows_amd import _ext
    return _ext


class Launch4(Launch):
    """``Launch`` whose mirrored rows go through usf_conv2d_same_pad_f32 with pad_before = 2 (the other rows: the public entry points)"""

    def __init__(self, c, d, B=None):
        super().__init__(c, d, B=B)
        self.c.mirror, self.c.pad_before = c.mirror, c.pad_before

    def run(self):
        c = self.c
        if not c.mirror:
            return super().run()
        ext = _ext()
        lib, p = ext.load(), (lambda t: None if t is None else t.data_ptr())
        n = c.B * c.cout * c.H * c.W
        lead = 1 if c.yoff else 0
        full = torch.full((lead + n + 2 * K.GUARD,), K.sentinel(), dtype=torch.float32, device=DEV)
        buf = full[lead:]
        y = buf.data_ptr() + 4 * K.GUARD
        assert (self.x.data_ptr() % 16 != 0) == c.xoff and (y % 16 != 0) == c.yoff and c.entry == "plain"
        rc = lib.usf_conv2d_same_pad_f32(self.x.data_ptr(), y, c.B, c.cin, c.cout, c.H, c.W, 4, c.pad_before, self.planes.data_ptr(),
                                         p(self.bias), p(self.in_mul), c.in_act, c.in_slope, c.out_act, c.out_slope, None, 0,
                                         ext.current_stream(torch.device(DEV)))
        torch.cuda.synchronize()
        return rc, buf


def _hold(name):
    c = CASES[name]
    a, got = _variant(c)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    assert got == c.expect, f"{name}: the probe answers {got} on this device ({cus} compute units), the table expects {c.expect} at 256"
    d = K.data(c)
    L = Launch4(c, d)
    rc, buf = L.run()
    if c.expect[0] == 0:
        assert rc == -3, rc                                           # refused: nothing is launched, nothing is written
        assert bool((K.bits(buf) == K.SENTINEL_BITS).all())
        return
    assert rc == 0, (rc, _ext().load().usf_last_error())
    ref64, A64 = K4.reference(c, L.on_device())
    found = K.check(c, buf, ref64, A64, bound=BOUND)
    print(f"{name}: kernel {a['kernel']} S {a['S']} worst {K.measure(c, L.y_of(buf), ref64, A64):.3f} U A of {BOUND} allowed")
    assert found == [], (name, found)
    y = L.y_of(buf)
    rc2, buf2 = L.run()
    assert rc2 == 0 and torch.equal(K.bits(buf2), K.bits(buf)), f"{name}: a second launch gives other bits"
    stem, m = (name[:-2], "_m") if name.endswith("_m") else (name, "")
    if stem.endswith("_b"):
        ca = CASES[stem[:-1] + "a" + m]
        assert K4.family(ca) == K4.family(c)
        La = Launch4(c, d, B=ca.B)
        rca, bufa = La.run()
        assert rca == 0 and torch.equal(K.bits(La.y_of(bufa)), K.bits(y[:ca.B])), f"{name}: batch (a)'s bits differ from batch (b)'s"


@pytest.mark.parametrize("name", [n for n, c in CASES.items() if c.expect[0] == 4])
def test_streamed_kernel(name):
    _hold(name)


@pytest.mark.parametrize("name", [n for n, c in CASES.items() if c.expect[0] in (0, 1)])
def test_resident_kernel_and_refusals(name):
    _hold(name)


def test_the_placement_argument_is_checked():
    """pad_before == 1 at ks = 4 and (ks - 1) / 2 at odd ks are the public call, bit for bit; every other value, and a gated call in
    the mirrored placement, is refused with an error code and writes nothing"""
    ext = _ext()
    lib = ext.load()
    st = ext.current_stream(torch.device(DEV))
    g = torch.Generator().manual_seed(3)
    for ks, cin, cout in ((4, 16, 32), (3, 5, 7), (5, 16, 16), (1, 8, 8)):
        x = torch.randn(9, cin, 7, 7, generator=g).to(DEV)
        planes = ext.conv2d_weight_planes(torch.randn(cout, cin, ks, ks, generator=g).to(DEV))
        same = ext.conv2d_same_pad(x, planes, cout, ks, (ks - 1) // 2)
        assert torch.equal(K.bits(same), K.bits(ext.conv2d_same(x, planes, cout, ks)))
        for pb in (-1, 0, 1, 2, 3, 4, 5):
            if pb in ((ks - 1) // 2, ks // 2):
                continue
            y = torch.full((9, cout, 7, 7), 7.0, device=DEV)
            rc = lib.usf_conv2d_same_pad_f32(x.data_ptr(), y.data_ptr(), 9, cin, cout, 7, 7, ks, pb, planes.data_ptr(), None, None, 0, 0.0, 0, 0.0,
                                             None, 0, st)
            torch.cuda.synchronize()
            assert rc < 0 and bool((y == 7.0).all()), (ks, pb, rc)
            assert lib.usf_conv2d_same_pad_fits(cin, cout, 7, 7, ks, pb) == 0
    x = torch.randn(4, 16, 7, 7, generator=g).to(DEV)
    planes = ext.conv2d_weight_planes(torch.randn(32, 16, 4, 4, generator=g).to(DEV))
    y, gx = torch.full((4, 16, 7, 7), 7.0, device=DEV), torch.randn(4, 16, 7, 7, device=DEV)
    rc = lib.usf_conv2d_same_pad_f32(x.data_ptr(), y.data_ptr(), 4, 16, 32, 7, 7, 4, 2, planes.data_ptr(), None, None, 0, 0.0, 0, 0.0,
                                     gx.data_ptr(), 16, st)
    torch.cuda.synchronize()
    assert rc < 0 and bool((y == 7.0).all())


@pytest.mark.parametrize("cin,cout,H,W,B", [(16, 32, 7, 7, 9), (64, 64, 7, 7, 5), (5, 7, 2, 3, 11), (64, 33, 16, 16, 2), (1, 7, 1, 1, 4)])
def test_mirrored_entry_is_the_data_gradient(cin, cout, H, W, B):
    """usf_conv2d_same_pad_f32 with pad_before = 2 on the flipped, transposed planes (usf_conv2d_weight_planes_f32, transposed = 1)
    against autograd's dx of the fp64 statement F.conv2d(F.pad(x, (1, 2, 1, 2)), w), every element inside MARGIN * K32_4 * U * A
    with A = the same sum over magnitudes"""
    ext = _ext()
    g = torch.Generator().manual_seed(cin * 1000 + cout)
    w = (torch.randn(cout, cin, 4, 4, generator=g) / (16 * cin) ** 0.5).to(DEV)
    dy = torch.randn(B, cout, H, W, generator=g).to(DEV)
    x = torch.zeros(B, cin, H, W, dtype=torch.float64, device=DEV, requires_grad=True)
    (F.conv2d(F.pad(x, (1, 2, 1, 2)), w.double()) * dy.double()).sum().backward()
    wt = w.double().flip(2, 3).transpose(0, 1)
    assert float((F.conv2d(F.pad(dy.double(), (2, 1, 2, 1)), wt) - x.grad).abs().max()) < 1e-12     # the identity itself, in fp64
    A = F.conv2d(F.pad(dy.double().abs(), (2, 1, 2, 1)), wt.abs())
    got = ext.conv2d_same_pad(dy, ext.conv2d_weight_planes(w, transposed=True), cin, 4, 2)
    torch.cuda.synchronize()
    ratio = ((got.double() - x.grad).abs() / (K.U * A)).max().item()
    print(f"dx {cin}->{cout} {H}x{W}: worst {ratio:.3f} U A of {BOUND} allowed")
    assert torch.isfinite(got).all() and ratio <= BOUND
    # ... and the forward placement on the same planes is NOT the gradient (the two placements differ by one position)
    if H * W > 1:
        other = ext.conv2d_same(dy, ext.conv2d_weight_planes(w, transposed=True), cin, 4)
        assert ((other.double() - x.grad).abs() / (K.U * A)).max().item() > BOUND


@pytest.mark.parametrize("cin,cout", [(1, 7), (5, 16), (16, 40), (33, 64), (64, 64)])
def test_device_weight_planes_at_ks4(cin, cout):
    """usf_conv2d_weight_planes_f32 at ks = 4, transposed 0 / 1 / 2, and the batch form: the bits of the planes built on the CPU
    from the header's layout text / of the flipped, transposed weight's planes, and of the binding's CPU formulation"""
    ext = _ext()
    c = K._case(("planes", "plain", 1, cin, cout, 2, 2, 4, "", "p0", (0,) * 6))
    w = K.data(c).w
    want, _ = K.planes(c, w, None)
    ct = K._case(("planes_t", "plain", 1, cout, cin, 2, 2, 4, "", "p0", (0,) * 6))
    want_t, _ = K.planes(ct, w.flip(2, 3).transpose(0, 1).contiguous(), None)
    same = lambda got, ref: got.shape == ref.shape and torch.equal(got.cpu().view(torch.int16), ref.view(torch.int16))
    wd = w.to(DEV)
    assert same(ext.conv2d_weight_planes(wd), want) and same(ext.conv2d_weight_planes(wd), ext.conv2d_weight_planes(w))
    assert same(ext.conv2d_weight_planes(wd, transposed=True), want_t)
    assert same(ext.conv2d_weight_planes(wd, transposed=True), ext.conv2d_weight_planes(w, transposed=True))
    pf, pt = ext.conv2d_weight_planes_pair(wd)
    assert same(pf, want) and same(pt, want_t)
    w3 = torch.randn(cout, cin, 3, 3, device=DEV)                      # a 3 x 3 weight in the same launch
    (bf, bt), (b3, b3t) = ext.WeightPlanesBatch([wd, w3]).run()
    torch.cuda.synchronize()
    assert same(bf, want) and same(bt, want_t)
    p3, p3t = ext.conv2d_weight_planes_pair(w3)
    assert torch.equal(b3.view(torch.int16), p3.view(torch.int16)) and torch.equal(b3t.view(torch.int16), p3t.view(torch.int16))


# ---- usf_conv_wgrad_k4_f32: the weight gradient at ks = 4 --------------------------------------------------------------------------
from wide_wgrad_cases import FORMS, inputs, xin64  # noqa: E402


def _check_grad(got, ref, what):
    scale = float(ref.abs().max())
    err = float((got.double() - ref).abs().max())
    tol = 2e-6 * scale                                                # the bound tests/test_wide_wgrad_gpu.py holds this arithmetic to
    print(f"{what}: max|ref| {scale:.3e} err {err:.3e} ({err / max(scale, 1e-300):.2e} rel) bound {tol:.3e}")
    assert torch.isfinite(got).all() and err <= tol, (what, err, tol)


@pytest.mark.parametrize("row", K4.WGRAD_ROWS, ids=lambda r: "x".join(map(str, r[0])))
def test_wgrad_k4_every_element_against_fp64(row):
    (cin, cout, H, W), nt = row
    ext = _ext()
    v = ext.conv_wgrad_k4_variant(300, cin, cout, H, W)
    assert v["served"] == 1 and v["tiles_per_wave"] == nt == K4.wgrad_tiles_per_wave(cin, cout) and v["position_parts"] == 4
    assert v["max_samples_per_block"] >= 3
    for B in K4.WGRAD_BATCHES:
        for form in FORMS:
            x, dy, kw = inputs(cin, cout, H, W, B, form, DEV)
            r = ext.conv_wgrad_k4(x, dy, **kw)
            assert r is not None, (row, B, form)
            dW, db = r
            rW, rb = K4.wgrad_ref64(x, dy, kw)
            _check_grad(dW, rW, f"{row[0]} B={B} {form} dW")
            assert dW.shape == (cout, cin, 4, 4)
            if kw.get("want_bias", True):
                _check_grad(db, rb, f"{row[0]} B={B} {form} db")
            else:
                assert db is None
            if form in ("plain", "presub_leaky"):                     # both forms, twice: the same bits
                again = ext.conv_wgrad_k4(x, dy, **kw)
                assert torch.equal(again[0], dW) and torch.equal(again[1], db), "a second launch gives other bits"


def test_wgrad_k4_is_autograds_gradient_of_the_same_convolution():
    """the statement of tests/conv4_cases.py IS torch's: fp64 autograd of nn.Conv2d(..., 4, padding="same")"""
    g = torch.Generator().manual_seed(0)
    x, dy = torch.randn(3, 5, 6, 7, generator=g, dtype=torch.float64), torch.randn(3, 4, 6, 7, generator=g, dtype=torch.float64)
    conv = torch.nn.Conv2d(5, 4, 4, padding="same").double()
    (conv(x) * dy).sum().backward()
    rW, rb = K4.wgrad_ref64(x, dy, {})
    assert float((rW - conv.weight.grad).abs().max()) < 1e-12 and float((rb - conv.bias.grad).abs().max()) < 1e-12
    dW, db = _ext().conv_wgrad_k4(x.float().to(DEV), dy.float().to(DEV))
    _check_grad(dW.cpu(), rW, "autograd dW")
    _check_grad(db.cpu(), rb, "autograd db")


def test_wgrad_k4_wrap_around_positions_are_exact_zeros():
    """x lives in the last two columns only, dy in the first two columns and in the first and last two rows: the taps that would
    wrap round a row end or leave the image meet the zero padding -- every tap equals fp64 exactly (small integers)"""
    ext = _ext()
    for cin, cout, H, W in [(4, 16, 14, 14), (16, 16, 16, 12), (5, 7, 9, 9), (16, 16, 5, 13), (3, 3, 2, 2)]:
        B = 3
        g = torch.Generator().manual_seed(H * W)
        x = torch.zeros(B, cin, H, W)
        x[:, :, :, max(W - 2, 0):] = torch.randint(1, 8, (B, cin, H, min(2, W)), generator=g).float()
        dy = torch.zeros(B, cout, H, W)
        dy[:, :, :, :2] = torch.randint(-4, 5, (B, cout, H, min(2, W)), generator=g).float()
        dy[:, :, :2, :] = torch.randint(-4, 5, (B, cout, min(2, H), W), generator=g).float()
        dy[:, :, max(H - 2, 0):, :] = torch.randint(-4, 5, (B, cout, min(2, H), W), generator=g).float()
        x, dy = x.to(DEV), dy.to(DEV)
        dW, db = ext.conv_wgrad_k4(x, dy)
        rW, rb = K4.wgrad_ref64(x, dy, {})
        assert torch.equal(dW.double(), rW) and torch.equal(db.double(), rb), (cin, cout, H, W)
        assert (rW != 0).any()


def test_wgrad_k4_refusals_write_nothing():
    ext = _ext()
    lib = ext.load()
    canary = 12345.0
    for cin, cout, H, W, ks in K4.WGRAD_REFUSED:
        assert lib.usf_conv_wgrad_k4_workspace(4, cin, cout, H, W, ks) == 0
        assert ext.conv_wgrad_k4_variant(4, cin, cout, H, W, ks)["served"] == 0
        x = torch.randn(4, cin, H, W, device=DEV)
        dy = torch.randn(4, cout, H, W, device=DEV)
        dW = torch.full((cout * cin * ks * ks,), canary, device=DEV)
        db = torch.full((cout,), canary, device=DEV)
        ws = torch.full((1 << 16,), canary, device=DEV)
        rc = lib.usf_conv_wgrad_k4_f32(x.data_ptr(), dy.data_ptr(), 4, cin, cout, H, W, ks, None, None, 0, 0.0, dW.data_ptr(), db.data_ptr(),
                                       ws.data_ptr(), ws.numel(), ext.current_stream(x.device))
        torch.cuda.synchronize()
        assert rc == 1 and (dW == canary).all() and (db == canary).all() and (ws == canary).all()
    # the other entry points keep refusing kernel 4
    x, dy = torch.randn(4, 16, 7, 7, device=DEV), torch.randn(4, 16, 7, 7, device=DEV)
    assert ext.conv_wgrad_wide(x, dy, 4) is None and lib.usf_conv_wgrad_workspace(4, 16, 16, 7, 7, 4) == 0
    assert lib.usf_conv_wgrad_k5_workspace(4, 16, 16, 7, 7, 4) == 0
    # a workspace one float short: an error, nothing launched
    need = lib.usf_conv_wgrad_k4_workspace(4, 16, 16, 7, 7, 4)
    dW, db, ws = torch.full((16 * 16 * 16,), canary, device=DEV), torch.full((16,), canary, device=DEV), torch.full((need,), canary, device=DEV)
    args = (x.data_ptr(), dy.data_ptr(), 4, 16, 16, 7, 7, 4, None, None, 0, 0.0, dW.data_ptr(), db.data_ptr(), ws.data_ptr())
    assert need > 0 and lib.usf_conv_wgrad_k4_f32(*args, need - 1, ext.current_stream(x.device)) < 0
    torch.cuda.synchronize()
    assert (dW == canary).all() and (db == canary).all() and (ws == canary).all()
    assert lib.usf_conv_wgrad_k4_f32(*args, need, ext.current_stream(x.device)) == 0
    torch.cuda.synchronize()
    assert not (dW == canary).any() and not (db == canary).any()


@pytest.mark.parametrize("row", K4.CTX_WGRAD_ROWS, ids=lambda r: "_".join(map(str, r)))
def test_ctx_wgrad_at_ks4_against_fp64(row):
    """usf_conv_ctx_wgrad_f32 with 16 taps: fp64 autograd of the context plane's convolution in torch's placement; fixed-order sums"""
    cout, H, W, stride, B = row
    ext = _ext()
    g = torch.Generator().manual_seed(cout * 100 + H * 10 + W + B)
    dy = torch.randn(B, cout, H, W, generator=g)
    ctx = 2.0 * torch.rand(B if stride else 1, generator=g)
    w = torch.zeros(cout, 1, 4, 4, dtype=torch.float64, requires_grad=True)
    plane = (ctx.double() if stride else ctx.double().expand(B)).reshape(-1, 1, 1, 1).expand(B, 1, H, W)
    (F.conv2d(F.pad(plane, (1, 2, 1, 2)), w) * dy.double()).sum().backward()
    ref = w.grad.reshape(cout, 16)
    got1 = ext.conv_ctx_wgrad(dy.to(DEV), ctx.to(DEV), 4)
    got2 = ext.conv_ctx_wgrad(dy.to(DEV), ctx.to(DEV), 4)
    torch.cuda.synchronize()
    assert torch.equal(got1, got2)
    _check_grad(got1.cpu(), ref, f"ctx wgrad {row}")
