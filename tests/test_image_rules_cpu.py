"""usflows_amd/image_rules.py, nothing launched: the rules answer what they answered before they were gathered there (recorded from
the parent commit on a host without a GPU and on one with an MI355X: tests/golden/routes/), the predicate and the dispatcher of the weight gradient walk one tuple, and GatedConv's
route is the pair of decisions it replaced."""
import functools
import itertools
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

KNOB_NAMES = ("wgrad_wide", "conv_k5", "conv_k4")


@pytest.fixture(scope="module")
def recorded():
    with open(R.FIXTURE) as f:
        assert tuple(json.load(f)["knob_order"]) == KNOB_NAMES
    rec = R.load()[R.host_name()]                 # (recorded without a device and with an MI355X)
    assert len(rec) == 8
    return rec


def _set(monkeypatch, knobs):
    for name, v in zip(KNOB_NAMES, knobs):
        monkeypatch.setattr(config, name, v)


def test_the_rules_answer_what_the_parent_commit_answered(recorded):
    got = R.answers(it, config)
    n = len(list(R.grid()))
    assert n == 6 * 6 * 8 * 4 * 2 * 2
    for key, want in recorded.items():
        assert sorted(got[key]) == sorted(want)
        for ks in R.KERNELS:
            assert {len(want[f"{rule}/ks{ks}"]) for rule in ("wgrad_served", "conv_same", "conv_int", "ctx_same", "ctx_int")} == {n // 4}
        assert len(want["pointwise_0/ks1"]) == len(want["pointwise_same/ks1"]) == n // 4
        assert len(want["refused"]) == 4 * len(R.refused_convs()) and "1" not in want["refused"]
        for rule, bits in want.items():
            if got[key][rule] != bits:
                first = next(i for i, (a, b) in enumerate(zip(got[key][rule], bits)) if a != b)
                pytest.fail(f"{rule} differs under knobs {key} at point {first} of its order")
    # the grid reaches both answers of every rule, and every kernel of the route
    for rule in ("wgrad_served", "conv_same", "conv_int", "ctx_same", "ctx_int", "pointwise_0", "pointwise_same", "gate_halves_0",
                 "gate_halves_same", "gated_tail", "channel_affine"):
        assert {"0", "1"} == set("".join(s for k in recorded for key, s in recorded[k].items() if key.split("/")[0] == rule)), rule


@pytest.mark.parametrize("knobs", R.KNOBS)
def test_route_predicate_and_dispatcher_are_one_rule(knobs, recorded, monkeypatch):
    """``wgrad_route`` is ``wgrad_served``, and ``conv_wgrad`` on stubbed bindings calls ``wgrad_kernels``' names in order, stops
    at the first that answers, answers exactly when the predicate says served, and hands defer / owners to the narrow one only"""
    _set(monkeypatch, knobs)
    lib = _ext.load()
    calls = []

    def stub(name, query, fixed_ks=None):
        def f(x, dy, *ks, **kw):
            k = fixed_ks if fixed_ks is not None else ks[0]
            assert (name == "narrow") == ("defer" in kw) == ("owners" in kw) and len(ks) == (fixed_ks is None)
            assert name != "narrow" or (kw["defer"] is True and kw["owners"] == (123,))
            assert sorted(set(kw) - {"defer", "owners"}) == ["in_act", "in_mul", "in_slope", "pre_sub", "want_bias"]
            calls.append(name)
            B, cin, H, W = x.shape
            return (name, k) if query(B, cin, dy.shape[1], H, W, k, kw["in_mul"] is not None) else None
        return f

    ws = lambda entry: lambda B, cin, cout, H, W, ks, masked: getattr(lib, entry)(B, cin, cout, H, W, ks) > 0
    narrow = lambda B, cin, cout, H, W, ks, masked: _ext.conv_wgrad_variant(B, cin, cout, H, W, ks, masked)["kernel"] != 0
    queries = {"narrow": narrow, "wide": ws("usf_conv_wgrad_wide_workspace"), "k5": ws("usf_conv_wgrad_k5_workspace"),
               "k4": ws("usf_conv_wgrad_k4_workspace")}
    monkeypatch.setattr(_ext, "conv_wgrad", stub("narrow", narrow))
    monkeypatch.setattr(_ext, "conv_wgrad_wide", stub("wide", queries["wide"]))
    monkeypatch.setattr(_ext, "conv_wgrad_k5", stub("k5", queries["k5"], 5))
    monkeypatch.setattr(_ext, "conv_wgrad_k4", stub("k4", queries["k4"], 4))
    tensor = functools.lru_cache(maxsize=None)(lambda *shape: torch.empty(*shape))
    rec = recorded["".join(str(int(k)) for k in knobs)]
    served_bits = {ks: iter(rec[f"wgrad_served/ks{ks}"]) for ks in R.KERNELS}
    seen = set()
    for cin, cout, (H, W), ks, masked, B in R.grid():
        served = next(served_bits[ks]) == "1"
        route = it.wgrad_route(B, cin, cout, H, W, ks, masked)
        assert (route is not None) == served == it.wgrad_served(B, cin, cout, H, W, ks, masked)
        names = image_rules.wgrad_kernels(ks, H * W)
        answering = [n for n in names if queries[n](B, cin, cout, H, W, ks, masked)]
        assert route == (answering[0] if answering else None)
        del calls[:]
        r = it.conv_wgrad(tensor(B, cin, H, W), tensor(B, cout, H, W), ks, in_mul=tensor(cin * H * W) if masked else None,
                          defer=True, owners=(123,))
        assert (r is not None) == served and (r is None or r == (route, ks))
        assert tuple(calls) == (names[:names.index(route) + 1] if served else names), (knobs, cin, cout, H, W, ks, masked, B)
        if not names:
            assert not calls and r is None          # knob off at kernel 4 / 5, wgrad_wide off above 64 pixels: no binding is asked
        seen.add((names, route))
    wide, k5, k4 = knobs
    assert ((), None) in seen or all(knobs)
    assert (("narrow",), "narrow") in seen or (("narrow", "wide"), "narrow") in seen
    assert ((("narrow", "wide"), "wide") in seen) == (wide and (k5 or k4))
    assert ((("wide",), "wide") in seen) == wide and ((("k5",), "k5") in seen) == k5 and ((("k4",), "k4") in seen) == k4


@pytest.mark.parametrize("knobs", R.KNOBS)
def test_wgrad_kernels_is_the_stated_table(knobs, monkeypatch):
    _set(monkeypatch, knobs)
    wide, k5, k4 = knobs
    for pixels in (1, 49, 64, 65, 256):
        assert image_rules.wgrad_kernels(5, pixels) == (("k5",) if k5 else ())
        assert image_rules.wgrad_kernels(4, pixels) == (("k4",) if k4 else ())
        for ks in (1, 3):
            if pixels >= 65:
                assert image_rules.wgrad_kernels(ks, pixels) == (("wide",) if wide else ())
            else:
                assert image_rules.wgrad_kernels(ks, pixels) == ("narrow",) + (("wide",) if wide and (k5 or k4) else ())
    assert image_rules.conv_kernel_sizes() == (1, 3) + ((4,) if k4 else ()) + ((5,) if k5 else ())
    assert it.WIDE_MIN_PIXELS == image_rules.WIDE_MIN_PIXELS == 65


@pytest.mark.parametrize("knobs", R.KNOBS)
def test_gate_conv_route_is_the_old_pair_of_decisions(knobs, monkeypatch):
    """None exactly where GatedConv.train_shape_ok's disjunction was false; the name by forward_train_device's order: the
    pointwise kernel, else the two halves where the convolution kernel does not take the shape and they do, else the convolution"""
    _set(monkeypatch, knobs)
    seen = set()
    for c, (H, W), B, pad in itertools.product(sorted(set((4,) + R.CHANNELS + R.GATE_C)), R.MAPS, R.BATCHES, (0, "same", 1)):
        conv = R._conv(c, 2 * c, 1, padding=pad)
        p, k, h = it.pointwise_shape_ok(conv, B, H, W), it.conv_shape_ok(conv, B, H, W), it.gate_halves_ok(conv, B, H, W)
        route = image_rules.gate_conv_route(conv, B, H, W)
        assert (route is not None) == (p or k or h)
        assert route == ("pointwise" if p else "halves" if (not k and h) else "conv" if k else None), (c, H, W, B, pad)
        seen.add(route)
    # (4 -> 8 channels: the pointwise kernel has no such instantiation, the wide weight gradient opens the convolution kernel)
    assert seen == {"pointwise", None} | ({"conv"} if knobs[0] else set()) | ({"halves"} if knobs[1] or knobs[2] else set())


def test_same_conv_ks_and_the_kernel_1_form(monkeypatch):
    _set(monkeypatch, (True, True, True))
    for ks in (1, 3, 4, 5):
        assert image_rules.same_conv_ks(R._conv(4, 4, ks, padding="same")) == ks
        assert image_rules.same_conv_ks(R._conv(4, 4, ks, padding=ks // 2)) == (ks if ks % 2 else 0)
    for name, conv in R.refused_convs():
        assert image_rules.same_conv_ks(conv) == 0 and not image_rules.pointwise_geometry(conv), name
    assert image_rules.same_conv_ks(torch.nn.Linear(4, 4)) == 0 and not image_rules.pointwise_geometry(torch.nn.Linear(4, 4))
    # the kernel-1 form does not look at dilation or padding mode (GatedConv hands its dilation to its 1 x 1 convolution)
    for conv in (R._conv(4, 8, 1, dilation=2), R._conv(4, 8, 1, padding_mode="reflect")):
        assert image_rules.pointwise_geometry(conv) and image_rules.same_conv_ks(conv) == 0
