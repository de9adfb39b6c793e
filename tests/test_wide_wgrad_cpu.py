"""usf_conv_wgrad_wide_f32 without a GPU: the plan covers every instantiation the kernel file has, the old weight-gradient
queries answer what they answered before the wide kernel existed, and the Python gates change above 64 pixels only."""
import itertools
import json
import os

import pytest
import torch

from usflows_amd import _ext, image_training as it
from usflows_amd.config import config
from wide_wgrad_cases import REFUSED, SHAPES, tiles_per_wave

HERE = os.path.dirname(os.path.abspath(__file__))
CHANNELS = (16, 24, 32, 48, 64)
MAPS = ((7, 7), (7, 8), (3, 19), (8, 8), (5, 13), (9, 9), (14, 14), (16, 16))     # 49, 56, 57, 64, 65, 81, 196, 256 pixels


def test_the_plan_covers_every_instantiation_and_only_those():
    have = sorted(_ext.conv_wgrad_wide_instances())
    need = {}
    for cit, cot, taps in itertools.product(range(1, 5), range(1, 5), (1, 9)):
        need.setdefault(tiles_per_wave(cit, cot, taps), []).append((cit, cot, taps))
    assert sorted(need) == have, (sorted(need), have)
    seen = set()
    for (cit, cot, taps), B in itertools.product([s for v in need.values() for s in v], (1, 32, 300, 5000)):
        ks = 3 if taps == 9 else 1
        for cin, cout in ((16 * cit, 16 * cot), (16 * cit - 15, 16 * cot - 3)):       # full tiles and ragged ones: the same plan
            v = _ext.conv_wgrad_wide_variant(B, cin, cout, 9, 9, ks, cus=256)
            assert v["served"] == 1 and (v["CIT"], v["COT"], v["T"]) == (cit, cot, taps)
            assert v["tiles"] == cot * (cit * taps + 1) and v["tiles_per_wave"] == tiles_per_wave(cit, cot, taps) in have
            assert v["wave_groups"] * v["position_parts"] == 4 and v["wave_groups"] * v["tiles_per_wave"] >= v["tiles"]
            assert v["blocks"] == min(B, 256 * min(v["blocks_per_cu"], 2)) and v["slots"] == v["blocks"] * v["position_parts"]
            assert v["max_samples_per_block"] == -(-B // v["blocks"]) and v["nacc"] == 256 * v["tiles"]
            assert v["rounds"] == (1 if v["slots"] <= 64 else 2) and v["per"] * v["rows_used"] >= v["slots"] and v["rows_used"] <= 64
            assert v["lds_bytes"] == 4 * ((16 * cit + 1) * v["CSx"] + 16 * cot * v["CSy"]) <= 160 * 1024
            for cs in (v["CSx"], v["CSy"]):
                assert cs % 2 == 0 and (cs // 2) % 2 == 1                             # 2 * odd: conflict-free fragment reads
            seen.add(v["tiles_per_wave"])
    assert sorted(seen) == have


def test_geometry_of_the_test_shapes_and_the_refusals():
    for cin, cout, H, W, ks in SHAPES:
        v = _ext.conv_wgrad_wide_variant(300, cin, cout, H, W, ks, cus=256)
        assert v["served"] == 1, (cin, cout, H, W, ks)
        S = W + 1 if ks == 3 else W
        n = (H - 1) * S + W
        assert v["S"] == S and v["nch"] == -(-n // 4) and v["CSy"] >= 4 * v["nch"]
        assert v["CSx"] >= (v["q0"] + 4 * v["nch"] + S + 1 if ks == 3 else 4 * v["nch"])
        assert _ext.load().usf_conv_wgrad_wide_workspace(300, cin, cout, H, W, ks) >= (v["slots"] + 64) * v["nacc"] > 0
    for cin, cout, H, W, ks in REFUSED:
        assert _ext.conv_wgrad_wide_variant(4, cin, cout, H, W, ks, cus=256)["served"] == 0
        assert _ext.load().usf_conv_wgrad_wide_workspace(4, cin, cout, H, W, ks) == 0
    # the one rule that refuses a shape inside the ranges: the sample's LDS image above 160 KiB
    assert _ext.conv_wgrad_wide_variant(4, 64, 64, 16, 16, 3, cus=256)["lds_bytes"] == 150744
    assert _ext.conv_wgrad_wide_variant(4, 64, 64, 128, 2, 3, cus=256)["served"] == 0
    assert _ext.conv_wgrad_wide_variant(4, 16, 16, 128, 2, 3, cus=256)["served"] == 1


def test_the_old_queries_answer_what_they_answered_before():
    """tests/golden/wide/old_wgrad_answers.json: usf_conv_wgrad_variant on the grid below, recorded from the weight-gradient
    planner as it was before the wide kernel was added"""
    gold = json.load(open(os.path.join(HERE, "golden", "wide", "old_wgrad_answers.json")))
    n = 0
    for cin, cout, (H, W), ks, masked, B in itertools.product(CHANNELS, CHANNELS, MAPS, (1, 3), (0, 1), (32, 300)):
        v = _ext.conv_wgrad_variant(B, cin, cout, H, W, ks, bool(masked), cus=gold["cus"], blocks_per_cu=gold["blocks_per_cu"])
        assert [v[k] for k in gold["fields"]] == gold["answers"][f"{B},{cin},{cout},{H},{W},{ks},{masked}"], (B, cin, cout, H, W, ks, masked)
        if H * W > 64:
            assert v["kernel"] == 0 and _ext.load().usf_conv_wgrad_workspace(B, cin, cout, H, W, ks) == 0
        n += 1
    assert n == len(gold["answers"]) == 1600


def _conv(cin, cout, ks):
    return torch.nn.Conv2d(cin, cout, ks, padding="same")


@pytest.mark.parametrize("knob", [True, False])
def test_the_gates_change_above_64_pixels_only(knob, monkeypatch):
    monkeypatch.setattr(config, "wgrad_wide", knob)
    lib = _ext.load()
    n_wide = 0
    for cin, cout, (H, W), ks, masked in itertools.product(CHANNELS, CHANNELS, MAPS, (1, 3), (False, True)):
        B = 32
        fits = lib.usf_conv2d_same_fits(cin, cout, H, W, ks) >= 2 and lib.usf_conv2d_same_fits(cout, cin, H, W, ks) >= 2
        old = _ext.conv_wgrad_variant(B, cin, cout, H, W, ks, masked)["kernel"] != 0
        wide = knob and lib.usf_conv_wgrad_wide_workspace(B, cin, cout, H, W, ks) > 0
        want = fits and (wide if H * W > 64 else old)
        assert it.conv_shape_ok(_conv(cin, cout, ks), B, H, W, masked=masked) == want, (cin, cout, H, W, ks, masked)
        assert it.wgrad_served(B, cin, cout, H, W, ks, masked) == (wide if H * W > 64 else old)
        n_wide += int(want and H * W > 64)
        if ks == 1 and not masked:
            pw = _ext.pointwise_conv_supported(cin, cout, False) and _ext.pointwise_conv_supported(cout, cin, False)
            ws_old = lib.usf_conv_wgrad_workspace(B, cin, cout, H, W, 1) > 0
            assert it.pointwise_shape_ok(_conv(cin, cout, 1), B, H, W) == (pw and (wide if H * W > 64 else ws_old))
        # conditional first convolutions stay declined above 64 pixels
        if H * W > 64:
            assert not it.conv_ctx_shape_ok(_conv(cin + 1, cout, ks), B, H, W)
    assert (n_wide > 0) == knob
