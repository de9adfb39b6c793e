"""usf_conv_wgrad_wide_f32 (feature maps of up to 256 pixels, any channel counts up to 64) against fp64, element by element.

Tolerance: the project's 2e-6 * max|ref| (test_conv_wgrad_vs_fp64).  These sums are up to four times longer, yet the worst
case measured is 6.7e-7 * max|ref| (300 rows of 256 pixels: 3e-7), so the bound is kept as it is.  Beside each error the test prints
the error a plain fp32 CPU computation of the same gradient (torch.nn.grad.conv2d_weight) makes against fp64 on the same inputs
(profiles/wide_wgrad_parity.md has both per case: tools/wide_wgrad_parity.py makes it from this file's output under -s)."""
import ctypes

import pytest
import torch

from usflows_amd import _ext
from wide_wgrad_cases import BATCHES, FORMS, MORE_SHAPES, REFUSED, SHAPES, err32, inputs, ref64, tiles_per_wave

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _check(got, ref, e32, what):
    scale = float(ref.abs().max())
    err = float((got.double() - ref).abs().max())
    tol = 2e-6 * scale
    print(f"{what}: max|ref| {scale:.3e} err {err:.3e} ({err / scale:.2e} rel) fp32-cpu err {e32:.3e} bound {tol:.3e}")
    assert torch.isfinite(got).all() and err <= tol, (what, err, tol)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_every_element_against_fp64(shape):
    cin, cout, H, W, ks = shape
    for B in BATCHES:
        for form in FORMS:
            x, dy, kw = inputs(cin, cout, H, W, B, form, DEV)
            r = _ext.conv_wgrad_wide(x, dy, ks, **kw)
            assert r is not None, (shape, B, form)
            dW, db = r
            rW, rb = ref64(x, dy, ks, kw)
            e32 = err32(x, dy, ks, kw)
            _check(dW, rW, e32, f"{shape} B={B} {form} dW")
            assert dW.shape == (cout, cin, ks, ks)
            if kw.get("want_bias", True):
                _check(db, rb, 0.0, f"{shape} B={B} {form} db")
            else:
                assert db is None


def test_every_instantiation_runs_on_the_device():
    """SHAPES and MORE_SHAPES together launch every tiles-per-wave instantiation the kernel file has, the largest LDS images
    (above 64 KiB: the raised dynamic-LDS limit) included; the further shapes at 5 and 300 rows, plain and with pre_sub + leaky"""
    launched = set()
    for cin, cout, H, W, ks in SHAPES + MORE_SHAPES:
        v = _ext.conv_wgrad_wide_variant(300, cin, cout, H, W, ks)
        assert v["served"] == 1 and v["tiles_per_wave"] == tiles_per_wave(-(-cin // 16), -(-cout // 16), ks * ks)
        launched.add(v["tiles_per_wave"])
    assert sorted(launched) == sorted(_ext.conv_wgrad_wide_instances())
    assert max(_ext.conv_wgrad_wide_variant(300, *s)["lds_bytes"] for s in MORE_SHAPES) == 150744
    for shape in MORE_SHAPES:
        cin, cout, H, W, ks = shape
        for B in (5, 300):
            for form in ("plain", "presub_leaky"):
                x, dy, kw = inputs(cin, cout, H, W, B, form, DEV)
                dW, db = _ext.conv_wgrad_wide(x, dy, ks, **kw)
                rW, rb = ref64(x, dy, ks, kw)
                _check(dW, rW, err32(x, dy, ks, kw), f"{shape} B={B} {form} dW")
                _check(db, rb, 0.0, f"{shape} B={B} {form} db")


def test_the_same_launch_twice_gives_the_same_bits():
    for cin, cout, H, W, ks, B in [(12, 16, 16, 16, 3, 300), (16, 16, 5, 13, 1, 33), (64, 64, 9, 9, 1, 5)]:
        x, dy, kw = inputs(cin, cout, H, W, B, "presub_leaky", DEV)
        a = _ext.conv_wgrad_wide(x, dy, ks, **kw)
        b = _ext.conv_wgrad_wide(x, dy, ks, **kw)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_wrap_around_positions_are_exact_zeros():
    """x lives in the last column only, dy in the first column and in the first and last rows: the taps that would wrap round a
    row end or leave the image meet the zero padding -- every tap equals fp64 exactly, zero where it is zero"""
    for cin, cout, H, W in [(4, 16, 14, 14), (16, 16, 16, 16), (5, 7, 9, 9), (16, 16, 5, 13)]:
        B = 3
        g = torch.Generator().manual_seed(H * W)
        x = torch.zeros(B, cin, H, W)
        x[:, :, :, W - 1] = torch.randint(1, 8, (B, cin, H), generator=g).float()
        dy = torch.zeros(B, cout, H, W)
        dy[:, :, :, 0] = torch.randint(-4, 5, (B, cout, H), generator=g).float()
        dy[:, :, 0, :] = torch.randint(-4, 5, (B, cout, W), generator=g).float()
        dy[:, :, H - 1, :] = torch.randint(-4, 5, (B, cout, W), generator=g).float()
        x, dy = x.to(DEV), dy.to(DEV)
        dW, db = _ext.conv_wgrad_wide(x, dy, 3)
        rW, rb = ref64(x, dy, 3, {})                                   # small integers: every sum is exact in fp32
        assert torch.equal(dW.double(), rW) and torch.equal(db.double(), rb)
        # kx = 0 reads the column left of p: to meet x (last column) p would lie one column past the row's end, where a
        # wrapping index finds dy's first column instead
        assert (rW[:, :, :, 0] == 0).all() and (rW != 0).any()


def test_a_small_map_agrees_with_the_narrow_kernel():
    cin, cout, H, W, ks = 32, 32, 7, 7, 3
    for B in (5, 300):
        x, dy, kw = inputs(cin, cout, H, W, B, "mask_relu_nobias", DEV)
        kw["want_bias"] = True
        wide = _ext.conv_wgrad_wide(x, dy, ks, **kw)
        narrow = _ext.conv_wgrad(x, dy, ks, **kw)
        assert wide is not None and narrow is not None
        for a, b in zip(wide, narrow):
            assert float((a - b).abs().max()) <= 2e-6 * float(b.abs().max())


def _raw_call(x, dy, cin, cout, H, W, ks, dW, db, ws, ws_n):
    B = x.shape[0]
    return _ext.load().usf_conv_wgrad_wide_f32(x.data_ptr(), dy.data_ptr(), B, cin, cout, H, W, ks, None, None, 0, 0.0, dW.data_ptr(),
                                               db.data_ptr(), ws.data_ptr(), ws_n, _ext.current_stream(x.device))


def test_refusals_write_nothing():
    lib = _ext.load()
    canary = 12345.0
    for cin, cout, H, W, ks in REFUSED:
        assert lib.usf_conv_wgrad_wide_workspace(4, cin, cout, H, W, ks) == 0
        assert _ext.conv_wgrad_wide_variant(4, cin, cout, H, W, ks)["served"] == 0
        x = torch.randn(4, cin, H, W, device=DEV)
        dy = torch.randn(4, cout, H, W, device=DEV)
        dW = torch.full((cout * cin * ks * ks,), canary, device=DEV)
        db = torch.full((cout,), canary, device=DEV)
        ws = torch.full((1 << 16,), canary, device=DEV)
        assert _raw_call(x, dy, cin, cout, H, W, ks, dW, db, ws, ws.numel()) == 1
        torch.cuda.synchronize()
        assert (dW == canary).all() and (db == canary).all() and (ws == canary).all()
        assert _ext.conv_wgrad_wide(x, dy, ks) is None
    # a workspace one float short: an error, nothing launched
    cin, cout, H, W, ks = 16, 16, 14, 14, 3
    need = lib.usf_conv_wgrad_wide_workspace(4, cin, cout, H, W, ks)
    assert need > 0
    x = torch.randn(4, cin, H, W, device=DEV)
    dy = torch.randn(4, cout, H, W, device=DEV)
    dW = torch.full((cout * cin * ks * ks,), canary, device=DEV)
    db = torch.full((cout,), canary, device=DEV)
    ws = torch.full((need,), canary, device=DEV)
    assert _raw_call(x, dy, cin, cout, H, W, ks, dW, db, ws, need - 1) < 0
    assert b"workspace too small" in lib.usf_last_error()
    torch.cuda.synchronize()
    assert (dW == canary).all() and (db == canary).all() and (ws == canary).all()
    assert _raw_call(x, dy, cin, cout, H, W, ks, dW, db, ws, need) == 0
    torch.cuda.synchronize()
    assert not (dW == canary).any() and not (db == canary).any()
    assert ctypes.sizeof(_ext.ConvWgradWideInfo) == lib.usf_sizeof_desc(24)
