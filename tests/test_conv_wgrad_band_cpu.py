"""usf_conv_wgrad_band_f32 without a GPU: the case table of tests/conv_wgrad_band_cases.py reaches every instantiation and
every regime of the plan (usf_conv_wgrad_band_variant at 256 compute units), refusals answer served 0 and workspace 0, the older
weight-gradient queries answer above 256 pixels what they answered before, the fp32 statements stay inside K * U * A, and the
multiply-high divisions of the staging loops are exact over the served range."""
import itertools

import numpy as np
import pytest

import conv_wgrad_band_cases as G
from usflows_amd import _ext


def _plan(row, cus=G.CUS):
    cin, cout, H, W, ks, rb, B, cap = row
    with G.block_cap(_ext.load(), cap):
        return _ext.conv_wgrad_band_variant(B, cin, cout, H, W, ks, band_rows=rb, cus=cus)


def test_the_table_reaches_every_instantiation_and_regime():
    plans = {G.name_of(r): _plan(r) for r in G.ROWS}
    assert all(v["served"] == 1 for v in plans.values())
    assert sorted({v["tiles_per_wave"] for v in plans.values()}) == sorted(_ext.conv_wgrad_band_instances())
    # one, several and ragged bands
    assert any(v["bands"] == 1 for v in plans.values())
    assert any(v["bands"] > 2 and v["last_rows"] == v["band_rows"] for v in plans.values())
    assert any(v["bands"] > 1 and v["last_rows"] < v["band_rows"] for v in plans.values())
    assert any(v["band_rows"] == 1 for v in plans.values()) and any(v["last_rows"] == 1 < v["band_rows"] for v in plans.values())
    # a band the plan kept at the LDS's size (above the 64 KiB a kernel gets unasked) beside the lowered ones
    assert any(v["lds_bytes"] > 64 * 1024 and v["band_rows"] == v["best_rows"] > 4 for v in plans.values())
    # grids below and at the cap, a block that walks several samples' bands, one and two reduction rounds, split position chunks
    assert any(v["grid"] == v["groups"] < G.CUS for v in plans.values())
    assert any(v["grid"] == G.CUS * min(v["blocks_per_cu"], 2) < v["groups"] for v in plans.values())
    assert any(v["grid"] == 2 and v["max_groups_per_block"] > 2 * v["bands"] for v in plans.values())
    assert {v["rounds"] for v in plans.values()} == {1, 2}
    assert any(v["position_parts"] == 2 for v in plans.values())
    v = plans[G.name_of(G.ROWS[0])]
    assert (v["band_rows"], v["bands"], v["last_rows"]) == (4, 5, 1)


def test_the_plan_is_consistent_over_the_served_range():
    """every field from the sizes alone, on a grid of shapes, batches and compute-unit counts"""
    inst = set(_ext.conv_wgrad_band_instances())
    n = 0
    for (cin, cout), (H, W), ks, B, cus, rb in itertools.product(
            [(1, 1), (3, 32), (32, 32), (33, 17), (64, 64), (16, 64)], [(28, 28), (32, 32), (17, 17), (64, 64), (4096, 1), (7, 64), (16, 16)],
            (1, 3), (1, 32, 1024), (104, 256), (0, 3)):
        v = _ext.conv_wgrad_band_variant(B, cin, cout, H, W, ks, band_rows=rb, cus=cus)
        ws = _ext.load().usf_conv_wgrad_band_workspace(B, cin, cout, H, W, ks, rb)
        if not v["served"]:
            assert ws == 0 and ks == 3 and min(cin, cout) > 16, (cin, cout, H, W, ks)     # the only refusal inside the ranges: no four rows fit
            continue
        n += 1
        cit, cot, T = -(-cin // 16), -(-cout // 16), ks * ks
        pad = ks // 2
        S = W + pad
        assert (v["CIT"], v["COT"], v["T"], v["S"]) == (cit, cot, T, S)
        assert 1 <= v["band_rows"] <= v["best_rows"] <= v["fit_rows"] <= H and (rb == 0 or v["band_rows"] <= rb)
        assert v["bands"] == -(-H // v["band_rows"]) and v["last_rows"] == H - (v["bands"] - 1) * v["band_rows"] >= 1
        assert v["staged_rows"] == v["band_rows"] + 2 * pad and v["groups"] == B * v["bands"]
        assert v["nch"] == -(-((v["band_rows"] - 1) * S + W) // 4) and v["CSy"] >= 4 * v["nch"]
        assert v["CSx"] >= (v["q0"] + 4 * v["nch"] + S + 1 if ks == 3 else 4 * v["nch"])
        for cs in (v["CSx"], v["CSy"]):
            assert cs % 2 == 0 and (cs // 2) % 2 == 1                                     # 2 * odd: conflict-free fragment reads
        assert v["lds_bytes"] == 4 * ((16 * cit + 1) * v["CSx"] + 64 + 16 * cot * v["CSy"]) <= 160 * 1024
        assert v["tiles"] == cot * (cit * T + 1) and v["tiles_per_wave"] in inst and v["nacc"] == 256 * v["tiles"]
        assert v["wave_groups"] * v["position_parts"] == 4 and v["wave_groups"] * v["tiles_per_wave"] >= v["tiles"]
        assert v["grid"] == min(v["groups"], cus * min(v["blocks_per_cu"], 2)) and v["slots"] == v["grid"] * v["position_parts"]
        assert v["max_groups_per_block"] == -(-v["groups"] // v["grid"])
        assert v["rounds"] == (1 if v["slots"] <= 64 else 2) and v["per"] * v["rows_used"] >= v["slots"] and v["rows_used"] <= 64
        # the low-batch rule: a lowered band only where the LDS-sized one leaves compute units without a group, never below 4 rows
        if v["best_rows"] < v["fit_rows"] and -(-H // v["fit_rows"]) != -(-H // v["best_rows"]):
            assert B * -(-H // v["fit_rows"]) < cus and v["best_rows"] >= 4
        if cus == 256:          # (the workspace query plans for the device's compute units: 256 where there is none)
            assert ws == (v["slots"] + 64) * v["nacc"] or _has_gpu()
    assert n > 500


def _has_gpu():
    import torch
    return torch.cuda.is_available()


def test_refusals_answer_not_served_and_no_workspace():
    lib = _ext.load()
    for cin, cout, H, W, ks in G.REFUSED:
        for B in (1, 4, 300):
            assert _ext.conv_wgrad_band_variant(B, cin, cout, H, W, ks, cus=G.CUS)["served"] == 0, (cin, cout, H, W, ks)
            assert lib.usf_conv_wgrad_band_workspace(B, cin, cout, H, W, ks, 0) == 0
    assert _ext.conv_wgrad_band_variant(0, 16, 16, 20, 20, 3, cus=G.CUS)["served"] == 0
    assert _ext.conv_wgrad_band_variant(4, 16, 16, 20, 20, 3, band_rows=-1, cus=G.CUS)["served"] == 0
    # the shape the flows' routing leaves on torch is served here: 64 -> 64 channels at 28 x 28 (the forward kernel refuses it)
    assert _ext.conv_wgrad_band_variant(32, 64, 64, 28, 28, 3, cus=G.CUS)["served"] == 1


def test_the_older_queries_answer_above_256_pixels_what_they_answered_before():
    lib = _ext.load()
    for (cin, cout), (H, W), ks, B in itertools.product([(16, 16), (32, 32), (3, 32), (64, 64)], [(28, 28), (32, 32), (17, 17), (1, 257)],
                                                        (1, 3), (1, 32, 300)):
        assert lib.usf_conv_wgrad_workspace(B, cin, cout, H, W, ks) == 0
        assert lib.usf_conv_wgrad_wide_workspace(B, cin, cout, H, W, ks) == 0
        assert _ext.conv_wgrad_variant(B, cin, cout, H, W, ks, cus=G.CUS, blocks_per_cu=1)["kernel"] == 0
        assert _ext.conv_wgrad_wide_variant(B, cin, cout, H, W, ks, cus=G.CUS)["served"] == 0


@pytest.mark.parametrize("row", G.ROWS, ids=G.name_of)
def test_the_fp32_statements_stay_inside_K(row):
    worst = [0.0] * 4
    for form in G.FORMS:
        worst = [max(a, b) for a, b in zip(worst, G.fp32_ratios(G.case(row, form)))]
    print(f"WGB-CPU {G.name_of(row)} dW {worst[0]:.3f} U A, db {worst[1]:.3f} U A, max-norm dW {worst[2]:.2e} db {worst[3]:.2e}")
    assert worst[0] <= G.K["dW"] and worst[1] <= G.K["db"]
    assert worst[2] < 1e-6 and worst[3] < 1e-6          # what lets the GPU file assert the suite's 2e-6


def test_the_multiply_high_divisions_are_exact():
    """n // d == (n * m) >> 32 for the plan's own m and EVERY dividend the kernel forms: e < channels * staged_rows * W with m_x
    (d = staged_rows * W), e < channels * band_rows * W with m_y, p < staged_rows * W with m_w -- over every W, every band height
    the served range allows at it and 64 channels (fewer channels form a subset of these dividends).  The band heights are a
    sample (the plan's own band, caps of 1, 2, 3 and half the map), so beside the enumeration every plan is held to the argument
    that covers ALL of them: m = ceil(2^32 / d) gives floor(n / d) exactly whenever n * d < 2^32 (the error term n (m d - 2^32) /
    (d 2^32) stays below 1 / d), and the plan's dividends stay below 64 * 4224 < 2^19, its divisors below 4224 < 2^13"""
    seen = 0
    for W in range(1, 65):
        heights = sorted({h for h in (1, 2, 3, 4, 5, 7, 8, 14, 15, 19, 28, 32, 63, 64, 100, 1000, 4096) if h * W <= 4096} | {4096 // W})
        for H, ks in itertools.product(heights, (1, 3)):
            for rb in sorted({0, 1, 2, 3, H // 2}):
                v = _ext.conv_wgrad_band_variant(1 << 18, 64, 64, H, W, ks, band_rows=rb, cus=G.CUS)
                if not v["served"]:
                    v = _ext.conv_wgrad_band_variant(1 << 18, 16, 16, H, W, ks, band_rows=rb, cus=G.CUS)
                assert v["served"] == 1
                dx, dy = v["staged_rows"] * W, v["band_rows"] * W
                assert v["max_dividend"] >= 16 * dx - 1
                assert 64 * dx * dx < 1 << 32 and 64 * dx * max(dy, W) < 1 << 32 and dx <= 4224      # n * d < 2^32 for every dividend
                e = np.arange(64 * dx, dtype=np.uint64)
                for d, m, top in ((dx, v["m_x"], 64 * dx), (dy, v["m_y"], 64 * dy), (W, v["m_w"], dx)):
                    n = e[:top]
                    got = n if m == 0 else (n * np.uint64(m)) >> np.uint64(32)
                    assert m == (0 if d == 1 else -(-(1 << 32) // d)) and bool((got == n // np.uint64(d)).all()), (W, H, ks, rb, d)
                seen += 1
    assert seen > 1000
