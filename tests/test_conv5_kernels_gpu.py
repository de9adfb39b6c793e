"""Every forward row of tests/conv5_cases.py launched once on the device and held to the fp64 statement on EVERY element, in
the manner of tests/test_conv_kernels_gpu.py (whose ``Launch`` builds the operands: NaN samples behind every input, sentinels in
front of and behind y): the probe's answer for this device, the per-element bound MARGIN * K32_5 * U * A next to the checker's
max-norm rule, the same bits from a second launch, batch (a) as a bit-exact prefix of batch (b); the device plane split at
ks = 5 against the builder's planes; usf_conv_wgrad_k5_f32 and the 25-tap usf_conv_ctx_wgrad_f32 against fp64 at
2e-6 * max|ref|, with the wrap-around and refusal tests of tests/test_wide_wgrad_gpu.py restated for two pad columns."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import conv_kernel_cases as K  # noqa: E402
import conv5_cases as K5  # noqa: E402
from test_conv_kernels_gpu import Launch, _variant, DEV  # noqa: E402

pytestmark = pytest.mark.gpu
CASES = {c.name: c for c in K5.cases()}
BOUND = K.MARGIN * K5.K32_5


def _ext():
    from usflows_amd import _ext
    return _ext


def _hold(name):
    c = CASES[name]
    a, got = _variant(c)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    assert got == c.expect, f"{name}: the probe answers {got} on this device ({cus} compute units), the table expects {c.expect} at 256"
    d = K.data(c)
    L = Launch(c, d)
    rc, buf = L.run()
    if c.expect[0] == 0:
        assert rc == -3, rc                                           # refused: nothing is launched, nothing is written
        assert bool((K.bits(buf) == K.SENTINEL_BITS).all())
        return
    assert rc == 0, (rc, _ext().load().usf_last_error())
    ref64, A64 = K.reference(c, L.on_device())
    found = K.check(c, buf, ref64, A64, bound=BOUND)
    print(f"{name}: kernel {a['kernel']} S {a['S']} worst {K.measure(c, L.y_of(buf), ref64, A64):.3f} U A of {BOUND} allowed")
    assert found == [], (name, found)
    y = L.y_of(buf)
    rc2, buf2 = L.run()
    assert rc2 == 0 and torch.equal(K.bits(buf2), K.bits(buf)), f"{name}: a second launch gives other bits"
    if name.endswith("_b"):
        ca = CASES[name[:-1] + "a"]
        assert K.family(ca) == K.family(c)
        La = Launch(c, d, B=ca.B)
        rca, bufa = La.run()
        assert rca == 0 and torch.equal(K.bits(La.y_of(bufa)), K.bits(y[:ca.B])), f"{name}: batch (a)'s bits differ from batch (b)'s"


@pytest.mark.parametrize("name", [n for n, c in CASES.items() if c.expect[0] == 4])
def test_streamed_kernel(name):
    _hold(name)


@pytest.mark.parametrize("name", [n for n, c in CASES.items() if c.expect[0] in (0, 1)])
def test_resident_kernel_and_refusals(name):
    _hold(name)


@pytest.mark.parametrize("cin,cout", [(1, 7), (5, 16), (16, 40), (33, 64), (64, 64)])
def test_device_weight_planes_at_ks5(cin, cout):
    """usf_conv2d_weight_planes_f32 at ks = 5, transposed 0 / 1 / 2, and the batch form: the bits of the planes built on the CPU
    from the header's layout text / of the flipped, transposed weight's planes"""
    ext = _ext()
    c = K._case(("planes", "plain", 1, cin, cout, 2, 2, 5, "", "p0", (0,) * 6))
    w = K.data(c).w
    want, _ = K.planes(c, w, None)
    ct = K._case(("planes_t", "plain", 1, cout, cin, 2, 2, 5, "", "p0", (0,) * 6))
    want_t, _ = K.planes(ct, w.flip(2, 3).transpose(0, 1).contiguous(), None)
    same = lambda got, ref: got.shape == ref.shape and torch.equal(got.cpu().view(torch.int16), ref.view(torch.int16))
    wd = w.to(DEV)
    assert same(ext.conv2d_weight_planes(wd), want)
    assert same(ext.conv2d_weight_planes(wd, transposed=True), want_t)
    pf, pt = ext.conv2d_weight_planes_pair(wd)
    assert same(pf, want) and same(pt, want_t)
    w3 = torch.randn(cout, cin, 3, 3, device=DEV)                      # a 3 x 3 weight in the same launch
    (bf, bt), (b3, b3t) = ext.WeightPlanesBatch([wd, w3]).run()
    torch.cuda.synchronize()
    assert same(bf, want) and same(bt, want_t)
    p3, p3t = ext.conv2d_weight_planes_pair(w3)
    assert torch.equal(b3.view(torch.int16), p3.view(torch.int16)) and torch.equal(b3t.view(torch.int16), p3t.view(torch.int16))


# ---- usf_conv_wgrad_k5_f32: the weight gradient at ks = 5 --------------------------------------------------------------------------
from wide_wgrad_cases import FORMS, err32, inputs, ref64  # noqa: E402


def _check_grad(got, ref, e32, what):
    scale = float(ref.abs().max())
    err = float((got.double() - ref).abs().max())
    tol = 2e-6 * scale                                                # the bound tests/test_wide_wgrad_gpu.py holds this arithmetic to
    print(f"{what}: max|ref| {scale:.3e} err {err:.3e} ({err / max(scale, 1e-300):.2e} rel) fp32-cpu err {e32:.3e} bound {tol:.3e}")
    assert torch.isfinite(got).all() and err <= tol, (what, err, tol)


@pytest.mark.parametrize("row", K5.WGRAD_ROWS, ids=lambda r: "x".join(map(str, r[0])))
def test_wgrad_k5_every_element_against_fp64(row):
    (cin, cout, H, W), nt = row
    ext = _ext()
    v = ext.conv_wgrad_k5_variant(300, cin, cout, H, W)
    assert v["served"] == 1 and v["tiles_per_wave"] == nt == K5.wgrad_tiles_per_wave(cin, cout) and v["position_parts"] == 5
    assert v["max_samples_per_block"] >= 3
    for B in K5.WGRAD_BATCHES:
        for form in FORMS:
            x, dy, kw = inputs(cin, cout, H, W, B, form, DEV)
            r = ext.conv_wgrad_k5(x, dy, **kw)
            assert r is not None, (row, B, form)
            dW, db = r
            rW, rb = ref64(x, dy, 5, kw)
            _check_grad(dW, rW, err32(x, dy, 5, kw) if B <= 5 else 0.0, f"{row[0]} B={B} {form} dW")
            assert dW.shape == (cout, cin, 5, 5)
            if kw.get("want_bias", True):
                _check_grad(db, rb, 0.0, f"{row[0]} B={B} {form} db")
            else:
                assert db is None
            if form == "presub_leaky":
                again = ext.conv_wgrad_k5(x, dy, **kw)
                assert torch.equal(again[0], dW) and torch.equal(again[1], db), "a second launch gives other bits"


def test_wgrad_k5_rows_launch_every_instantiation():
    ext = _ext()
    assert sorted({nt for _, nt in K5.WGRAD_ROWS}) == sorted(ext.conv_wgrad_k5_instances())


def test_wgrad_k5_wrap_around_positions_are_exact_zeros():
    """x lives in the last two columns only, dy in the first two columns and in the first and last two rows: the taps that would
    wrap round a row end by one or two positions or leave the image meet the zero padding -- every tap equals fp64 exactly"""
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
        dW, db = ext.conv_wgrad_k5(x, dy)
        rW, rb = ref64(x, dy, 5, {})                                   # small integers: every sum is exact in fp32
        assert torch.equal(dW.double(), rW) and torch.equal(db.double(), rb), (cin, cout, H, W)
        if W >= 6:
            # kx = 0, 1 read two / one columns left of p: to meet x (the last two columns) p would lie past the row's end,
            # where a wrapping index finds dy's first columns instead
            assert (rW[:, :, :, 0] == 0).all() and (rW != 0).any()


def test_wgrad_k5_refusals_write_nothing():
    ext = _ext()
    lib = ext.load()
    canary = 12345.0
    for cin, cout, H, W, ks in K5.WGRAD_REFUSED:
        assert lib.usf_conv_wgrad_k5_workspace(4, cin, cout, H, W, ks) == 0
        assert ext.conv_wgrad_k5_variant(4, cin, cout, H, W, ks)["served"] == 0
        x = torch.randn(4, cin, H, W, device=DEV)
        dy = torch.randn(4, cout, H, W, device=DEV)
        dW = torch.full((cout * cin * ks * ks,), canary, device=DEV)
        db = torch.full((cout,), canary, device=DEV)
        ws = torch.full((1 << 16,), canary, device=DEV)
        rc = lib.usf_conv_wgrad_k5_f32(x.data_ptr(), dy.data_ptr(), 4, cin, cout, H, W, ks, None, None, 0, 0.0, dW.data_ptr(), db.data_ptr(),
                                       ws.data_ptr(), ws.numel(), ext.current_stream(x.device))
        torch.cuda.synchronize()
        assert rc == 1 and (dW == canary).all() and (db == canary).all() and (ws == canary).all()
    # the existing entry points keep refusing kernel 5
    x, dy = torch.randn(4, 16, 7, 7, device=DEV), torch.randn(4, 16, 7, 7, device=DEV)
    assert ext.conv_wgrad_wide(x, dy, 5) is None and lib.usf_conv_wgrad_workspace(4, 16, 16, 7, 7, 5) == 0
    # a workspace one float short: an error, nothing launched
    need = lib.usf_conv_wgrad_k5_workspace(4, 16, 16, 7, 7, 5)
    dW, db, ws = torch.full((16 * 16 * 25,), canary, device=DEV), torch.full((16,), canary, device=DEV), torch.full((need,), canary, device=DEV)
    args = (x.data_ptr(), dy.data_ptr(), 4, 16, 16, 7, 7, 5, None, None, 0, 0.0, dW.data_ptr(), db.data_ptr(), ws.data_ptr())
    assert need > 0 and lib.usf_conv_wgrad_k5_f32(*args, need - 1, ext.current_stream(x.device)) < 0
    torch.cuda.synchronize()
    assert (dW == canary).all() and (db == canary).all() and (ws == canary).all()
    assert lib.usf_conv_wgrad_k5_f32(*args, need, ext.current_stream(x.device)) == 0
    torch.cuda.synchronize()
    assert not (dW == canary).any() and not (db == canary).any()


@pytest.mark.parametrize("row", K5.CTX_WGRAD_ROWS, ids=lambda r: "_".join(map(str, r)))
def test_ctx_wgrad_at_ks5_against_fp64(row):
    """usf_conv_ctx_wgrad_f32 with 25 taps: fp64 autograd of the context plane's convolution; fixed-order sums"""
    import torch.nn.functional as F
    cout, H, W, stride, B = row
    ext = _ext()
    g = torch.Generator().manual_seed(cout * 100 + H * 10 + W + B)
    dy = torch.randn(B, cout, H, W, generator=g)
    ctx = 2.0 * torch.rand(B if stride else 1, generator=g)
    w = torch.zeros(cout, 1, 5, 5, dtype=torch.float64, requires_grad=True)
    plane = (ctx.double() if stride else ctx.double().expand(B)).reshape(-1, 1, 1, 1).expand(B, 1, H, W)
    (F.conv2d(plane, w, padding=2) * dy.double()).sum().backward()
    ref = w.grad.reshape(cout, 25)
    got1 = ext.conv_ctx_wgrad(dy.to(DEV), ctx.to(DEV), 5)
    got2 = ext.conv_ctx_wgrad(dy.to(DEV), ctx.to(DEV), 5)
    torch.cuda.synchronize()
    assert torch.equal(got1, got2)
    _check_grad(got1.cpu(), ref, 0.0, f"ctx wgrad {row}")
