"""The knob ``train_band`` in usflows_amd/image_rules.py, nothing launched.  Off (as shipped): every rule answers what the
parent commit answered on the recorded grid (tests/golden/routes/) and declines every map above 256 pixels.  On: the recorded
grid -- which has no map above 256 pixels -- answers the same, maps of 257 .. 4096 pixels go to usf_conv_wgrad_band_f32 and the
row-banded convolution in both directions, and ``conv_wgrad`` calls that kernel and only it."""
import json
import os
import sys

import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden", "routes"))
import record_image_rules as R  # noqa: E402
from usflows_amd import _ext, image_rules, image_training as it  # noqa: E402
from usflows_amd.config import config  # noqa: E402

LARGE = ((28, 28), (32, 32))
SERVED = ((1, 32), (32, 32), (32, 1), (3, 32))       # cin -> cout of the MNIST / CIFAR conditioners at c_hidden 32


def _conv(cin, cout, ks):
    return torch.nn.Conv2d(cin, cout, ks, padding="same", device="meta")


@pytest.mark.parametrize("knob", [False, True])
def test_the_recorded_grid_answers_what_the_parent_commit_answered(knob, monkeypatch):
    assert config.train_band is False                     # ships off
    monkeypatch.setattr(config, "train_band", knob)
    assert max(H * W for H, W in R.MAPS) == 256           # the grid has no map above 256 pixels: the knob may not move it
    with open(R.FIXTURE) as f:
        json.load(f)
    recorded = R.load()[R.host_name()]
    got = R.answers(it, config)
    for key, want in recorded.items():
        assert got[key] == want, key


def test_knob_off_declines_every_map_above_256_pixels():
    assert not config.train_band
    for (H, W), (cin, cout), ks, B in ((m, c, k, b) for m in LARGE for c in SERVED for k in (1, 3) for b in (1, 32, 1024)):
        assert not it.conv_shape_ok(_conv(cin, cout, ks), B, H, W) and not it.wgrad_served(B, cin, cout, H, W, ks, False)
        assert not it.wgrad_served(B, cin, cout, H, W, ks, True)
    for ks, pixels in ((1, 257), (3, 784), (3, 4096)):
        assert image_rules.wgrad_kernels(ks, pixels) == ("wide",)
    assert image_rules.gate_conv_route(_conv(32, 64, 1), 32, 28, 28) is None
    assert "band" in image_rules.WGRAD_KERNELS


def test_knob_on_routes_maps_above_256_pixels_to_the_band_kernels(monkeypatch):
    before = {(ks, p): image_rules.wgrad_kernels(ks, p) for ks in (1, 3, 4, 5) for p in (49, 64, 65, 256, 257, 784, 4096)}
    monkeypatch.setattr(config, "train_band", True)
    for ks in (1, 3):
        for p in (257, 784, 4096):
            assert image_rules.wgrad_kernels(ks, p) == ("band",)
        for p in (49, 64, 65, 256):
            assert image_rules.wgrad_kernels(ks, p) == before[ks, p]
    for ks in (4, 5):
        for p in (49, 256, 257, 784, 4096):
            assert image_rules.wgrad_kernels(ks, p) == before[ks, p]
    for (H, W) in LARGE:
        for cin, cout in SERVED:
            for B in (1, 32, 1024):
                assert it.conv_shape_ok(_conv(cin, cout, 3), B, H, W), (cin, cout, H, W)
                assert it.conv_shape_ok(_conv(cin, cout, 3), B, H, W, masked=True)
                assert it.wgrad_route(B, cin, cout, H, W, 3, True) == "band"
        assert not it.conv_shape_ok(_conv(64, 64, 3), 32, H, W)            # no four rows beside the weight planes: torch
        assert not it.conv_shape_ok(_conv(32, 32, 5), 32, H, W) and not it.conv_shape_ok(_conv(32, 32, 4), 32, H, W)
        # GatedConv's 1 x 1 convolution 32 -> 64 trains, on the pointwise kernel or the matrix-core convolution
        assert image_rules.gate_conv_route(_conv(32, 64, 1), 32, H, W) in ("pointwise", "conv")
        assert it.pointwise_shape_ok(_conv(32, 64, 1), 32, H, W) == \
            (_ext.pointwise_conv_supported(32, 64, False) and _ext.pointwise_conv_supported(64, 32, False))
        # conditional first convolutions stay declined above 64 pixels
        for cin, cout in SERVED:
            assert not it.conv_ctx_shape_ok(_conv(cin + 1, cout, 3), 32, H, W)
        assert not it.conv_ctx_shape_ok(_conv(2, 32, 3), 32, 9, 9)
        # the affine blocks: C <= 12 as before (usf_channel_affine_bwd_f32), C = 16 .. 64 reach the new kernel through wgrad_served
        for C in (1, 3, 12):
            assert it.channel_affine_train_ok(R._DeviceInput(32, C, H, W), C)
        for C in (16, 32, 48, 64):
            assert it.channel_affine_train_ok(R._DeviceInput(32, C, H, W), C)
        assert not it.channel_affine_train_ok(R._DeviceInput(32, 24, H, W), 24)
    # a map wider than 64 and one above 4096 pixels stay on torch
    assert not it.conv_shape_ok(_conv(32, 32, 3), 32, 4, 65) and not it.conv_shape_ok(_conv(32, 32, 3), 32, 65, 64)
    # without the inference knob there is no forward kernel: declined
    monkeypatch.setattr(config, "conv_band", False)
    assert not it.conv_shape_ok(_conv(32, 32, 3), 32, 28, 28)


def test_the_fused_forms_decline_maps_above_256_pixels():
    """conv2d_same_res / conv2d_same_gate answer None there (their planner picks no kernel), so the two-pass fallbacks of
    image_training run"""
    for entry in ("res", "gate_mul", "gate_add"):
        for cin, cout in SERVED:
            for H, W in LARGE:
                assert _ext.conv2d_same_variant(entry, 32, cin, cout, H, W, 3, cus=256)["kernel"] == 0


def test_conv_wgrad_calls_the_band_kernel_and_only_it(monkeypatch):
    monkeypatch.setattr(config, "train_band", True)
    calls = []

    def stub(name):
        def f(x, dy, *a, **kw):
            calls.append((name, a, sorted(kw)))
            return (name, None)
        return f

    for name in ("conv_wgrad", "conv_wgrad_wide", "conv_wgrad_k5", "conv_wgrad_k4"):
        monkeypatch.setattr(_ext, name, stub(name))
    monkeypatch.setattr(_ext, "conv_wgrad_band", stub("band"))
    x, dy = torch.empty(2, 32, 28, 28, device="meta"), torch.empty(2, 32, 28, 28, device="meta")
    assert image_rules.conv_wgrad(x, dy, 3, defer=True, owners=(1,)) == ("band", None)
    assert calls == [("band", (3,), ["in_act", "in_mul", "in_slope", "pre_sub", "want_bias"])]
    # a refusal is handed on as None: no other kernel is tried above 256 pixels
    monkeypatch.setattr(_ext, "conv_wgrad_band", lambda *a, **kw: None)
    assert image_rules.conv_wgrad(x, dy, 1) is None and len(calls) == 1
    # below 257 pixels the knob changes nothing
    x, dy = torch.empty(2, 32, 16, 16, device="meta"), torch.empty(2, 32, 16, 16, device="meta")
    assert image_rules.conv_wgrad(x, dy, 3)[0] == "conv_wgrad_wide"
