"""What tests/test_conv_band_kernels_gpu.py rests on, proved without a GPU: the table of tests/conv_band_cases.py launches both
instantiations of conv2d_same_band_kernel in every patch shape and every kind of band (computed from
usf_conv2d_same_band_variant's answers for 256 compute units, never by hand), the checker reports the planted defects on a
multi-band case and passes the fp32 statement, the plan reproduces the issue's figures and refuses what it should, the kernel's
magic-number division is exact over its reach, and the knob, the routing rule and the older queries answer as stated."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import conv_band_cases as T  # noqa: E402
from usflows_amd import _ext, image_rules  # noqa: E402
from usflows_amd.config import config  # noqa: E402

CUS = 256


@pytest.fixture(scope="module")
def lib():
    if not _ext.lib_exists():
        import __graft_entry__
        __graft_entry__.build()
    return _ext.load()


def _plan(c, band_rows, B=None):
    return _ext.conv2d_same_band_variant(c.B if B is None else B, c.cin, c.cout, c.H, c.W, c.ks, ctx=c.entry == "ctx", band_rows=band_rows,
                                         cus=CUS)


def test_the_table_covers_what_it_claims(lib):
    cs = T.cases()
    names = [c.name for c in cs]
    assert len(set(names)) == len(names) and len(cs) <= 40
    cover, caps = {}, set()
    for c in cs:
        for br in c.band_rows:
            a = _plan(c, br)
            assert a["served"] == 1 and a["stage_iters"] <= 16 and a["lds_bytes"] <= 158 * 1024, (c.name, br, a)
            assert a["band_rows"] == (min(br, a["best_rows"]) if br else a["best_rows"]) and a["groups"] == c.B * a["bands"]
            assert a["bands"] == -(-c.H // a["band_rows"]) and a["last_rows"] == c.H - (a["bands"] - 1) * a["band_rows"]
            assert a["grid"] == min(a["groups"], CUS) and a["CTX"] == (c.entry == "ctx")
            caps.add(br)
            for kind in T.band_kinds(c.H, a["band_rows"]):
                shape = (a["PC_last"], a["PR_last"]) if kind in ("last", "ragged_last") else (a["PC_full"], a["PR_full"])
                cover.setdefault((a["CTX"], shape), set()).add(kind)
    # both instantiations x the three patch shapes a launch without gated mode has, each in a first, an interior, a full last
    # and a ragged last band
    assert set(cover) == {(ctx, s) for ctx in (0, 1) for s in ((1, 1), (1, 2), (2, 2))}
    for key, kinds in cover.items():
        assert kinds >= {"first", "interior", "last", "ragged_last"}, (key, kinds)
    assert caps == set(T.BAND_ROWS)
    # the shapes and sizes the issue names
    shapes = {(c.H, c.W) for c in cs}
    assert {(17, 17), (52, 5), (5, 64), (28, 28), (32, 32), (7, 7), (8, 8), (16, 16)} <= shapes and any(w == 1 for _, w in shapes)
    assert {1, 3, 9, 32} <= {c.cin for c in cs if c.ks == 3} and 64 in {c.cin for c in cs if c.ks == 1}
    assert {1, 3, 17, 32, 64} <= {c.cout for c in cs} and {1, 2, 31} <= {c.B for c in cs}
    for hw in ((28, 28), (32, 32)):
        assert sum(1 for c in cs if (c.cin, c.cout, c.H, c.W) == (32, 32) + hw and c.band_rows == (0,)) == 1
    # the stale-halo case: 527 groups on 256 blocks, one row per band, 32 -> 32 channels
    stale = next(c for c in cs if c.name == "plain_32_32_17x17_stale")
    a = _plan(stale, 1)
    assert (a["groups"], a["grid"], a["bands"]) == (527, 256, 17) and stale.B * stale.cout * 17 * 17 * 4 < 1.2e6
    # forms: both context strides, a checkerboard-like 0 / 1 mask, masked channels, every activation pairing, with and without bias
    assert {c.ctx_stride for c in cs if c.entry == "ctx"} == {0, 1}
    assert {c.get("in_mul") for c in cs} >= {None, "rand", "chan"} and {bool(c.get("bias")) for c in cs} == {True, False}
    assert {(c.in_act, c.out_act) for c in cs} == {(T.K.LEAKY, T.K.NONE), (T.K.NONE, T.K.LEAKY), (T.K.LEAKY, T.K.LEAKY), (T.K.NONE, T.K.NONE)}
    # (d) of the GPU file: three shapes the resident-sample kernel serves too
    small = [c for c in cs if c.H * c.W <= 256]
    assert {(c.H, c.W) for c in small} == {(7, 7), (8, 8), (16, 16)}
    for c in small:
        assert lib.usf_conv2d_same_fits(c.cin, c.cout, c.H, c.W, c.ks) >= 1


def test_the_plan_reproduces_the_issues_figures(lib):
    for shape, (wbytes, best, bands) in T.PLAN_FIGURES.items():
        a = _ext.conv2d_same_band_variant(1, *shape, cus=CUS)
        assert (a["served"], a["weight_bytes"], a["best_rows"], a["band_rows"], a["bands"]) == (1, wbytes, best, best, bands), (shape, a)
        assert lib.usf_conv2d_same_band_fits(*shape) == best
    # 12 rows at 28 x 28 and 10 at 32 x 32 are what the LDS leaves; 8 rows at 64 -> 64, kernel 1 are what the 16 staged iterations leave
    a = _ext.conv2d_same_band_variant(1, 64, 64, 32, 32, 1, cus=CUS)
    assert a["stage_iters"] == 16 and a["lds_bytes"] + 3 * 32 * 9 * 16 <= 158 * 1024
    for shape, wbytes in (((48, 48, 32, 32, 3), 131328), ((64, 64, 32, 32, 3), 224256)):
        a = _ext.conv2d_same_band_variant(1, *shape, cus=CUS)
        assert (a["served"], a["weight_bytes"], a["best_rows"]) == (0, wbytes, 0)


def test_the_refusals(lib):
    for shape in T.REFUSED:
        assert lib.usf_conv2d_same_band_fits(*shape) == 0, shape
        assert _ext.conv2d_same_band_variant(4, *shape, cus=CUS)["served"] == 0, shape
    # a best band of 3 rows at kernel 3 is refused; the same map at kernel 1 (no halo) is not, nor a whole map of 3 rows
    a = _ext.conv2d_same_band_variant(4, *T.REFUSED_3_ROWS, cus=CUS)
    assert (a["served"], a["best_rows"]) == (0, 3) and lib.usf_conv2d_same_band_fits(*T.REFUSED_3_ROWS) == 0
    assert lib.usf_conv2d_same_band_fits(40, 40, 32, 32, 1) > 0 and lib.usf_conv2d_same_band_fits(40, 40, 3, 32, 3) == 3
    # the edges of the served range
    for shape in ((64, 64, 64, 64, 1), (1, 1, 4096, 1, 3), (64, 8, 32, 32, 3), (8, 64, 64, 64, 3)):
        assert lib.usf_conv2d_same_band_fits(*shape) > 0, shape
    # bad arguments are errors before any pointer is looked at, B == 0 is nothing to do, a refused shape is answered 1
    call = lambda B, cin, band_rows=0, in_act=0: lib.usf_conv2d_same_band_f32(None, None, B, cin, 8, 17, 17, 3, None, None, None, in_act, 0.0, 0,
                                                                             0.0, None, 0, None, band_rows, None)
    assert call(0, 8) == 0 and call(4, 65) == 1 and call(4, 8) == -1 and call(-1, 8) == -2 and call(4, 8, -1) == -2 and call(4, 8, 0, 7) == -2
    assert b"usf_conv2d_same_band_f32" in lib.usf_last_error()


def test_every_served_plan_stays_inside_its_limits(lib):
    """over a grid of the served range: LDS within 158 KiB, at most 16 staged iterations, the capped band never above the plan's"""
    n = 0
    for cin in (1, 3, 8, 9, 16, 17, 32, 33, 48, 64):
        for cout in (1, 16, 17, 32, 48, 64):
            for H, W in ((17, 17), (28, 28), (32, 32), (64, 64), (4096, 1), (64, 1), (5, 64), (100, 40), (1, 64), (3, 64)):
                for ks in (1, 3):
                    best = lib.usf_conv2d_same_band_fits(cin, cout, H, W, ks)
                    for br in (0, 1, 5, 16):
                        a = _ext.conv2d_same_band_variant(3, cin, cout, H, W, ks, band_rows=br, cus=CUS)
                        assert a["served"] == (best > 0)
                        if best:
                            n += 1
                            assert 1 <= a["band_rows"] <= min(best, H) and a["lds_bytes"] <= 158 * 1024 and a["stage_iters"] <= 16
                            assert best >= min(4, H) or ks == 1
                            pos = (a["band_rows"] + ks - 1) * (W + ks - 1)
                            assert a["lds_bytes"] == a["weight_bytes"] + 3 * pos * (((cin + 7) // 8) | 1) * 16
    assert n > 1000


def test_the_magic_number_division_is_exact_over_its_reach():
    """umulhi(n, floor(2^32 / W) + 1) == n // W for every pixel index of a served map (n < 4096), W = 2 .. 64 (W = 1 divides by nothing)"""
    n = np.arange(4096 + 64, dtype=np.uint64)
    for W in range(2, 65):
        m = (((1 << 32) // W) & 0xFFFFFFFF) + 1
        assert np.array_equal((n * np.uint64(m)) >> np.uint64(32), n // np.uint64(W)), W


# ---- the checker ---------------------------------------------------------------------------------------------------------
def _result(c, y):
    buf, n = T.guarded(c)
    buf[T.GUARD:T.GUARD + n] = y.float().flatten()
    return buf


@pytest.mark.parametrize("defect", T.DEFECTS)
def test_the_checker_reports_a_planted_defect_on_a_multi_band_case(lib, defect):
    c = next(c for c in T.cases() if c.name == "plain_3_17_17x17")
    assert min(_plan(c, br)["bands"] for br in c.band_rows if br) >= 2
    d = T.data(c)
    ref64, A64 = T.reference(c, d)
    assert T.check(c, _result(c, ref64), ref64, A64, T.BOUND) == []
    found = T.check(c, _result(c, T.forward(c, d, torch.float64, defect=defect)[0]), ref64, A64, T.BOUND)
    assert found and any("over" in f for f in found), found


def test_the_fp32_statement_passes_and_stays_inside_k32():
    """the k32 figure of THIS table, measured as conv_kernel_cases measured its own: the fp32 statement against the fp64 one,
    worst element; the module's K32 is that maximum rounded up in the second digit, not a loose cap"""
    worst = {}
    for c in T.cases():
        d = T.data(c)
        ref64, A64 = T.reference(c, d)
        y32 = T.forward(c, d, torch.float32)[0]
        r = T.measure(c, y32, ref64, A64)
        worst[c.entry] = max(worst.get(c.entry, (0.0, ""))[0], r), (c.name if r >= worst.get(c.entry, (0.0, ""))[0] else worst[c.entry][1])
        assert r <= T.K32, (c.name, r)
        assert T.check(c, _result(c, y32), ref64, A64, T.BOUND) == [], c.name
    print("k32 per entry:", {k: (round(v[0], 3), v[1]) for k, v in worst.items()})
    assert 0.5 * T.K32 < max(v[0] for v in worst.values()) <= T.K32 and T.BOUND == T.MARGIN * T.K32


# ---- the knob, the routing rule, the older queries ------------------------------------------------------------------------
def test_the_knob_and_the_routing_rule(lib, monkeypatch):
    assert "conv_band" in config._KNOBS and isinstance(config._KNOBS["conv_band"], bool)
    served = [(1, 32, 28, 28, 3), (32, 32, 28, 28, 3), (32, 64, 28, 28, 1), (3, 32, 32, 32, 3), (32, 32, 64, 64, 3), (16, 16, 17, 17, 3)]
    monkeypatch.setattr(config, "conv_band", False)
    assert not any(image_rules.band_conv_ok(*s) for s in served)
    monkeypatch.setattr(config, "conv_band", True)
    assert all(image_rules.band_conv_ok(*s) for s in served)
    # 256 pixels and fewer stay with usf_conv2d_same_f32; what the plan refuses stays on torch; kernels 4 and 5 too
    for s in ((32, 32, 16, 16, 3), (16, 16, 7, 7, 3), (64, 64, 32, 32, 3), (48, 48, 28, 28, 3), T.REFUSED_3_ROWS, (8, 8, 28, 28, 5), (8, 8, 28, 28, 4)):
        assert not image_rules.band_conv_ok(*s), s
    # the layer rule of networks.py follows it; training keeps asking usf_conv2d_same_fits alone
    from usflows_amd import networks
    conv = torch.nn.Conv2d(32, 32, 3, padding="same")
    assert not image_rules.conv_shape_ok(conv, 32, 28, 28) and not image_rules.conv_ctx_shape_ok(conv, 32, 28, 28)
    assert networks.band_conv_ok is image_rules.band_conv_ok


def test_the_old_queries_answer_what_they_answered_before(lib):
    """usf_conv2d_same_fits / _pad_fits / _variant around 256 pixels: nothing above 256 pixels, the first kernel's formula below"""
    q, out = _ext.ConvVariantQuery(), _ext.ConvVariant()
    for cin, cout in ((1, 32), (16, 16), (32, 32), (64, 64)):
        for H, W in ((16, 16), (15, 17), (17, 15), (16, 17), (17, 17), (1, 256), (1, 257), (28, 28), (32, 32), (64, 64)):
            for ks in (1, 3, 4, 5):
                fits = lib.usf_conv2d_same_fits(cin, cout, H, W, ks)
                assert lib.usf_conv2d_same_pad_fits(cin, cout, H, W, ks, (ks - 1) // 2) == fits
                for e in ("plain", "ctx", "res", "gate_mul", "gate_add"):
                    q.entry, q.aligned, q.B, q.cin, q.cout, q.H, q.W, q.ks, q.cus = _ext.CONV_ENTRIES[e], 1, 100, cin, cout, H, W, ks, CUS
                    assert lib.usf_conv2d_same_variant(q, out) == 0
                    if H * W > 256:
                        assert fits == 0 and out.kernel == 0, (cin, cout, H, W, ks, e)
                    elif e in ("plain", "ctx"):
                        assert (out.kernel != 0) == (fits > 0)
                if H * W <= 256 and ks in (1, 3):
                    # the first kernel's rule, restated: the most samples (at most 8) whose images fit 158 KiB beside the weights
                    cp, coutp = (cin + 7) // 8 * 8, (cout + 15) // 16 * 16
                    kp = (ks * ks * cp + 31) // 32 * 32
                    lds = lambda S: 3 * coutp * ((kp // 8) | 1) * 16 + 3 * S * (H + ks - 1) * (W + ks - 1) * ((cp // 8) | 1) * 16
                    it = lambda S: ((S * ((cin + 1) // 2) + 7) // 8) * ((H * W + 63) // 64)
                    want = next((S for S in range(8, 0, -1) if lds(S) <= 158 * 1024 and it(S) <= 16), 0)
                    assert fits == want, (cin, cout, H, W, ks)
    # the call itself still refuses such maps with its error, not with a launch
    assert lib.usf_conv2d_same_f32(None, None, 4, 8, 8, 17, 17, 3, None, None, None, 0, 0.0, 0, 0.0, None, 0, None) == -2
    assert lib.usf_abi_version() == 36
