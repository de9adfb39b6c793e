"""The fp32 side buffer of the planes inference plans, host side (no GPU): which affine GEMMs of a launch list hand the transformed
half of their output to the fused coupling behind them as fp32 (usf_gemm_planes_side / usf_coupling_planes_side),
with which block ranges; that knob planes_side_f32 = 0 builds the plain list; the list interpreted on the CPU
(tests/emulator_side.py, whose GEMM poisons the planes blocks the kernel no longer writes) against the plain list's result; and
the entry points' argument checks, which run before any launch."""
import ctypes

import pytest
import torch

import emulator
import emulator_side
from model_util import build_flow
from oracle import usflows_oracle as orc
from usflows_amd import _ext
from usflows_amd.engine import FlowEngine


def _engine(D, hidden=(24, 16), K=2, soft=False, side=True, fused_min_rows=0):
    spec = orc.FlowSpec(D, K, list(hidden), householder=0, soft_training=soft)
    eng = FlowEngine(build_flow(spec, orc.synth_state_dict(spec, seed=2)).layers)
    eng.use_planes, eng.planes_min_rows, eng.fused_min_rows = True, 0, fused_min_rows
    eng.planes_side_f32, eng.planes_side_min_rows = side, 0
    return eng


def _ops(plan):
    return [plan["arr"][j] for j in range(plan["n"])]


def _side_pairs(plan):
    """[(side_kb0, side_kbn, both_kb0, both_kbn)] of the list's GEMM prefix ops; checks that every one stands in front of a GEMM
    that is followed by a coupling prefix with the same buffer and block count and that coupling's op"""
    ops, out = _ops(plan), []
    for j, op in enumerate(ops):
        if op.kind == _ext.OP_CALL and op.u.call.fn == _ext.FN_GEMM_PLANES_SIDE:
            a = [int(op.u.call.a[i]) for i in range(5)]
            assert op.u.call.n_args == 5 and ops[j + 1].kind == _ext.OP_GEMM_PLANES
            c = ops[j + 2]
            assert c.kind == _ext.OP_CALL and c.u.call.fn == _ext.FN_COUPLING_PLANES_SIDE and c.u.call.n_args == 2
            assert int(c.u.call.a[0]) == a[0] and int(c.u.call.a[1]) == a[2]
            cd = ops[j + 3].u.coupling_planes
            assert ops[j + 3].kind == _ext.OP_COUPLING_PLANES and (cd.kb_t0, cd.nk_t) == (a[1], a[2])
            g = ops[j + 1].u.gemm_planes
            assert g.C_planes == cd.z and g.c_kb0 == 0 and g.c_kbn == cd.z_nkb and not g.residual
            # the blocks written both ways are exactly those the coupling's first layer reads
            both = set(range(a[3], a[3] + a[4]))
            assert both == set(range(cd.kb_t0, cd.kb_t0 + cd.nk_t)) & set(range(cd.kb_p0, cd.kb_p0 + cd.nk_p))
            assert a[0] % 16 == 0 and plan["ws"]["pside"].data_ptr() == a[0]
            assert plan["ws"]["pside"].numel() >= -(-cd.M // 16) * cd.nk_t * 2048
            out.append(tuple(a[1:]))
    n_cpl = sum(1 for op in ops if op.kind == _ext.OP_CALL and op.u.call.fn == _ext.FN_COUPLING_PLANES_SIDE)
    assert n_cpl == len(out)
    return out


def _n_calls(plan):
    return sum(1 for op in _ops(plan) if op.kind == _ext.OP_CALL)


@pytest.mark.parametrize("direction", ["backward", "forward"])
@pytest.mark.parametrize("D,expect", [
    (72, [(0, 2, 1, 1), (1, 2, 1, 1)]),        # 36 | 36: block 1 holds conditioning and transformed features; the masks alternate
    (64, [(0, 1, 0, 0), (1, 1, 1, 0)]),        # 32 | 32: no straddling block
    (200, [(0, 4, 3, 1), (3, 4, 3, 1)])])      # 100 | 100: blocks 0..3 resp. 3..6, block 3 straddles
def test_side_ranges_of_an_inference_plan(D, expect, direction, monkeypatch):
    emulator.install_prep_emulation(monkeypatch)
    eng = _engine(D)
    plan = eng._plan(direction, 48, torch.device("cpu"), False, "user")
    assert plan.get("planes")
    pairs = _side_pairs(plan)
    n_fused = sum(1 for op in _ops(plan) if op.kind == _ext.OP_COUPLING_PLANES)
    # every coupling of these flows stands behind an affine layer: each gets its residual as fp32, log_prob and sample direction
    assert n_fused == 2 and sorted(pairs) == expect
    assert _n_calls(plan) == 2 * n_fused


def test_knob_off_builds_the_plain_list(monkeypatch):
    emulator.install_prep_emulation(monkeypatch)
    on = _engine(72)._plan("backward", 48, torch.device("cpu"), False, "user")
    eng = _engine(72, side=False)
    off = eng._plan("backward", 48, torch.device("cpu"), False, "user")
    assert _n_calls(off) == 0 and "pside" not in off["ws"]
    # ... and the list with the side buffer is that list plus the prefix ops: same kinds, same shapes, in the same order
    rest = [op for op in _ops(on) if op.kind != _ext.OP_CALL]
    assert [op.kind for op in rest] == [op.kind for op in _ops(off)]
    for a, b in zip(rest, _ops(off)):
        if a.kind == _ext.OP_GEMM_PLANES:
            ga, gb = a.u.gemm_planes, b.u.gemm_planes
            assert (ga.M, ga.nk, ga.a_nkb, ga.c_nkb, ga.c_kb0, ga.c_kbn, ga.N) == (gb.M, gb.nk, gb.a_nkb, gb.c_nkb, gb.c_kb0, gb.c_kbn, gb.N)
        elif a.kind == _ext.OP_COUPLING_PLANES:
            ca, cb = a.u.coupling_planes, b.u.coupling_planes
            assert (ca.M, ca.kb_p0, ca.nk_p, ca.kb_t0, ca.nk_t, ca.sign) == (cb.M, cb.kb_p0, cb.nk_p, cb.kb_t0, cb.nk_t, cb.sign)
    # below planes_side_min_rows a forced plan keeps the plain list as well, and the two settings are different plans
    eng = _engine(72)
    eng.planes_side_min_rows = 8192
    assert _n_calls(eng._plan("backward", 48, torch.device("cpu"), False, "user")) == 0
    eng.planes_side_min_rows = 0
    assert _n_calls(eng._plan("backward", 48, torch.device("cpu"), False, "user")) == 4


def test_chained_training_and_context_plans_keep_the_plain_list(monkeypatch):
    emulator.install_prep_emulation(monkeypatch)
    dev = torch.device("cpu")
    # a coupling below the fused kernel's cross-over is a chain of GEMMs whose last one reads the residual from the planes
    chained = _engine(72, fused_min_rows=1000)._plan("backward", 48, dev, False, "user")
    assert chained.get("planes") and _n_calls(chained) == 0
    assert not any(op.kind == _ext.OP_COUPLING_PLANES for op in _ops(chained))
    # a training plan keeps every layer's planes buffer whole: the backward pass reads it
    eng = _engine(128, hidden=(24, 16))
    eng.train_planes_min_rows, eng.gemm_mode = 0, "bf16x3"
    if eng._planes_ok("backward", 48, False, True):
        train = eng._plan("backward", 48, dev, False, "nat", train=True)
        assert train.get("planes_train") and _n_calls(train) == 0
    # a flow with a context: its couplings run as usf_coupling_planes_ctx launches, which keep the residual in the planes; the
    # same flow run WITHOUT a context has plain fused couplings and gets the side buffer
    eng = _engine(72, soft=True)
    with_ctx = eng._plan("backward", 48, dev, True, "user")
    assert with_ctx.get("planes") and with_ctx["has_ctx"]
    assert all(_ext.is_ctx_prefix(op) for op in _ops(with_ctx) if op.kind == _ext.OP_CALL) and _n_calls(with_ctx) == 2
    assert _side_pairs(with_ctx) == []
    without = eng._plan("backward", 48, dev, False, "user")
    assert sorted(_side_pairs(without)) == [(0, 2, 1, 1), (1, 2, 1, 1)]


@pytest.mark.parametrize("fmt", ["bf16x3", "f16x2"])
@pytest.mark.parametrize("D,B", [(72, 100), (64, 40)])
def test_emulated_plan_with_the_side_buffer_gives_the_plain_plans_bits(D, B, fmt, monkeypatch):
    """both directions through the interpreter: the GEMM's side blocks leave as fp32 and their planes are poisoned (NaN) unless
    the coupling's first layer reads them; the result is the plain list's, bit for bit, and finite"""
    emulator.install_prep_emulation(monkeypatch)
    seen = emulator_side.register(monkeypatch)
    x = torch.rand(B, D, generator=torch.Generator().manual_seed(5))
    outs = {}
    for side in (True, False):
        eng = _engine(D, side=side)
        for direction in ("backward", "forward"):
            outs[side, direction] = emulator.engine_transform(eng, x, direction, None, True, planes=fmt)
        assert any(_n_calls(p) > 0 for p in eng._plans.values()) == side
    assert seen.gemm == 4 and seen.coupling == 4
    for direction in ("backward", "forward"):
        assert torch.isfinite(outs[True, direction]).all()
        assert torch.equal(outs[True, direction], outs[False, direction])


def _gemm_desc():
    """a planes-output descriptor that passes usf_gemm_planes_bf16x3's own checks (no pointer is read: validation comes first)"""
    g = _ext.GemmPlanesDesc()
    g.A, g.a_nkb, g.a_kb0, g.nk, g.M = 0x100000, 3, 0, 3, 100
    g.W_planes, g.ldw, g.w_plane_stride, g.w_rows = 0x200000, 96, 96 * 96, 96
    g.C_planes, g.c_nkb, g.c_kb0, g.c_kbn = 0x300000, 3, 0, 3
    g.res_sign, g.format = 1.0, _ext.PLANES_BF16X3
    return g


def _cpl_desc():
    d = _ext.CouplingPlanesDesc()
    d.z, d.z_nkb, d.M = 0x100000, 4, 40
    d.kb_p0, d.nk_p, d.kb_t0, d.nk_t = 0, 2, 1, 3
    d.n_hidden, d.hidden_padded = 1, 256
    d.W_in, d.ldw_in, d.w_in_plane, d.b_in = 0x200000, 64, 256 * 64, 0x300000
    d.W_out, d.ldw_out, d.w_out_plane, d.b_out = 0x400000, 256, 96 * 256, 0x500000
    d.sign, d.slope, d.act, d.format = 1.0, 0.01, _ext.ACT_LEAKY_RELU, _ext.PLANES_BF16X3
    return d


@pytest.mark.parametrize("what,kw,rc,msg", [
    ("null side", dict(side=None), -1, b"null side"),
    ("misaligned side", dict(side=0x800008), -2, b"16-byte aligned"),
    ("empty range", dict(rng=(1, 0, 1, 0)), -2, b"bad block ranges"),
    ("negative start", dict(rng=(-1, 2, 0, 0)), -2, b"bad block ranges"),
    ("range past the output", dict(rng=(2, 2, 2, 0)), -2, b"bad block ranges"),
    ("both range outside the side range", dict(rng=(1, 2, 0, 1)), -2, b"bad block ranges"),
    ("both range past the side range", dict(rng=(1, 1, 1, 2)), -2, b"bad block ranges"),
    ("residual", dict(residual=0x900000), -2, b"no residual"),
    ("fp32 output", dict(f32=True), -2, b"planes output"),
    ("4 GiB", dict(M=16 * (1 << 20), rng=(1, 2, 1, 0)), -3, b"side buffer larger"),
])
def test_gemm_side_argument_errors_are_reported_without_a_gpu(what, kw, rc, msg):
    lib = _ext.load()
    g = _gemm_desc()
    if "residual" in kw:
        g.residual = kw["residual"]
    if kw.get("f32"):
        g.C_planes, g.C_f32, g.ldc, g.N = 0, 0xA00000, 96, 96
    if "M" in kw:
        g.M, g.a_nkb, g.nk, g.c_nkb = kw["M"], 1, 1, 3       # (the operand itself stays below its own limit: a one-block K)
    got = lib.usf_gemm_planes_side(ctypes.byref(g), kw.get("side", 0x800000), *kw.get("rng", (1, 2, 1, 1)), None)
    assert got == rc and msg in lib.usf_last_error(), (what, got, lib.usf_last_error())


@pytest.mark.parametrize("what,kw,rc,msg", [
    ("null side", dict(side=None), -1, b"null side"),
    ("misaligned side", dict(side=0x800004), -2, b"16-byte aligned"),
    ("block count", dict(nkb=2), -2, b"blocks per panel"),
    ("hidden_out", dict(hidden_out=0x600000), -2, b"inference launch"),
])
def test_coupling_side_argument_errors_are_reported_without_a_gpu(what, kw, rc, msg):
    lib = _ext.load()
    d = _cpl_desc()
    if "hidden_out" in kw:
        d.hidden_out[0] = kw["hidden_out"]
    nkb = kw.get("nkb", d.nk_t)
    got = lib.usf_coupling_planes_side(ctypes.byref(d), kw.get("side", 0x800000), nkb, None)
    assert got == rc and msg in lib.usf_last_error(), (what, got, lib.usf_last_error())


def test_side_prefix_ops_need_their_planes_op():
    """inside an op list the side buffer rides in a USF_OP_CALL op that applies to the planes op behind it: a list that ends behind
    the prefix, continues with another kind of op, or carries a bad range is rejected before anything is launched"""
    lib = _ext.load()
    buf = torch.zeros(4096)
    arr = (_ext.Op * 2)()
    arr[0] = _ext.gemm_planes_side_prefix(buf, 1, 2, 1, 1)
    assert _ext.is_side_prefix(arr[0]) and not _ext.is_ctx_prefix(arr[0]) and not _ext.is_side_prefix(arr[1])
    assert lib.usf_run_ops(arr, 1, None) == -2 and b"USF_FN_GEMM_PLANES_SIDE" in lib.usf_last_error()
    arr[1].kind = _ext.OP_COUPLING_PLANES
    assert lib.usf_run_ops(arr, 2, None) == -2 and b"USF_FN_GEMM_PLANES_SIDE" in lib.usf_last_error()
    arr[1].kind = _ext.OP_GEMM_PLANES
    arr[1].u.gemm_planes = _gemm_desc()
    arr[0].u.call.a[2] = 5                                  # the side range runs past the output's three blocks
    assert lib.usf_run_ops(arr, 2, None) == -2 and b"bad block ranges" in lib.usf_last_error()
    arr[0] = _ext.coupling_planes_side_prefix(buf, 3)
    assert _ext.is_side_prefix(arr[0])
    assert lib.usf_run_ops(arr, 1, None) == -2 and b"USF_FN_COUPLING_PLANES_SIDE" in lib.usf_last_error()
    assert lib.usf_run_ops(arr, 2, None) == -2 and b"USF_FN_COUPLING_PLANES_SIDE" in lib.usf_last_error()
    arr[1].kind = _ext.OP_COUPLING_PLANES
    arr[1].u.coupling_planes = _cpl_desc()
    arr[0].u.call.a[1] = 2                                  # the layer transforms three blocks
    assert lib.usf_run_ops(arr, 2, None) == -2 and b"blocks per panel" in lib.usf_last_error()
