"""usf_channel_affine_bwd_f32 without a GPU: the case table of channel_affine_bwd_cases.py launches every instantiation, loops
and sums in more than one step somewhere, the refusals are refusals -- all from the variant query, which launches nothing -- and a
numpy fp32 statement of the kernel's summation order stays within 1e-6 of max|ref| of fp64 on every case: the 2e-6 the device
test allows does not rest on the code under test."""
import ctypes

import pytest
import torch

from usflows_amd import _ext
from channel_affine_bwd_cases import CASES, EMU_TOL, MULTI_TRIP_C1, REFUSED, aligned, case_id, check, emulate, inputs, ref64, wants


def plan(case):
    B, C, P, form, cap = case
    return _ext.channel_affine_bwd_variant(B, C, P, aligned=aligned(case), want_bias=wants(case)[2], grid_cap=cap)


def test_the_table_launches_every_instantiation():
    seen = set()
    for case in CASES:
        v = plan(case)
        B, C, P, form, cap = case
        assert v["served"] == 1 and v["width"] == -(-C // 4) * 4 and v["vec"] == int(aligned(case) and P % 4 == 0), case
        assert v["slot_floats"] == C * C + (C if wants(case)[2] else 0) and v["slots"] == v["blocks"] <= 256
        units = B * P // 4 if v["vec"] else B * P
        assert v["blocks"] == min(-(-units // 256), cap or 256) and v["trips"] == -(-units // (256 * v["blocks"]))
        assert _ext.load().usf_channel_affine_bwd_workspace(B, C, P) >= v["blocks"] * v["slot_floats"] + 64 * v["slot_floats"]
        seen.add((v["width"], v["vec"]))
    assert seen == {(w, f) for w in (4, 8, 12) for f in (0, 1)}
    # every width, full and ragged, in both forms; with and without each optional operand
    assert {(c[1], plan(c)["vec"]) for c in CASES} >= {(C, f) for C in (1, 3, 4, 5, 8, 9, 12) for f in (0, 1)}
    assert {wants(c) for c in CASES} == {(False, True, True), (True, True, True), (True, False, True), (False, True, False)}


def test_the_table_has_several_trips_and_two_rounds_in_both_forms():
    trips = {(plan(c)["vec"], plan(c)["width"]) for c in CASES if plan(c)["trips"] > 1}
    assert trips >= {(1, 4), (1, 8), (1, 12), (0, 4), (0, 8), (0, 12)}
    assert {plan(c)["vec"] for c in CASES if plan(c)["rounds"] == 2} == {0, 1}
    v = plan(MULTI_TRIP_C1)
    assert (v["trips"], v["blocks"], v["rounds"], v["per"], v["rows_used"], v["vec"]) == (2, 256, 2, 16, 16, 1)
    # a batch whose pixels are no multiple of a block's 256 units: the last block is partly idle
    assert any((c[0] * c[2] // (4 if plan(c)["vec"] else 1)) % 256 for c in CASES)


def test_the_grid_is_a_function_of_the_sizes():
    """the same sizes plan the same grid whatever was asked before; the cap only ever lowers it"""
    a = _ext.channel_affine_bwd_variant(1024, 4, 196)
    assert (a["blocks"], a["trips"], a["rounds"], a["grid_cap"]) == (196, 1, 2, 256)
    assert _ext.channel_affine_bwd_variant(1024, 4, 196, grid_cap=7)["blocks"] == 7
    assert _ext.channel_affine_bwd_variant(1024, 4, 196, grid_cap=100000)["blocks"] == 196
    assert _ext.channel_affine_bwd_variant(1024, 4, 196) == a
    assert _ext.channel_affine_bwd_variant(1 << 20, 12, 256)["blocks"] == 256


def test_refusals():
    lib = _ext.load()
    for B, C, P in REFUSED + [(4, 13, 196), (4, 4, 0)]:          # C = 13 and P = 0 by name
        assert lib.usf_channel_affine_bwd_workspace(B, C, P) == 0, (B, C, P)
        assert _ext.channel_affine_bwd_variant(B, C, P)["served"] == 0
        # the entry point itself: 1, before any pointer is looked at (no GPU here: nothing may be launched)
        assert lib.usf_channel_affine_bwd_f32(None, None, None, B, C, P, None, None, None, None, None, 0, None, None) == 1
    # an empty batch is a no-op
    assert lib.usf_channel_affine_bwd_f32(None, None, None, 0, 4, 196, None, None, None, None, None, 0, None, None) == 0
    assert ctypes.sizeof(_ext.ChannelAffineBwdQuery) == lib.usf_sizeof_desc(25)
    assert ctypes.sizeof(_ext.ChannelAffineBwdInfo) == lib.usf_sizeof_desc(26)


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_the_summation_order_in_fp32_stays_within_1e_6_of_fp64(case):
    x, dy, W, ps = inputs(case)
    _, rW, rb = ref64(x, dy, W, ps)
    v = plan(case)
    v = dict(v, slot_floats=case[1] * case[1] + case[1])          # (the statement always carries db)
    dW, db = emulate(x, dy, ps, v)
    check(torch.from_numpy(dW), rW, f"{case_id(case)} dW (fp32 order)", EMU_TOL)
    check(torch.from_numpy(db), rb, f"{case_id(case)} db (fp32 order)", EMU_TOL)
