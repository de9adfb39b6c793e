"""A context on the planes pipeline, host side (no GPU): the planes plan of a conditional / soft-trained flat flow -- the prefix op
that turns a fused coupling launch into usf_coupling_planes_ctx, the context vectors, the base density in the last GEMM's epilogue,
the training step's context-layer gradients -- interpreted on the CPU (tests/emulator_ctx.py) against the reference's goldens and
the fp64 oracle; and the entry point's argument checks, which run before any launch."""
import ctypes

import pytest
import torch

import emulator
import emulator_ctx
from golden_util import load_case
from model_util import build_flow
from oracle import usflows_oracle as orc
from usflows_amd import _ext
from usflows_amd.engine import FlowEngine

FMT = {"bf16x3": 0, "f16x2": 1}


def _ctx_plans(eng):
    return [p for p in eng._plans.values() if p.get("planes") and p.get("has_ctx")]


def _has_ctx_launch(plan):
    arr = plan["arr"]
    return any(_ext.is_ctx_prefix(arr[j]) and arr[j + 1].kind == _ext.OP_COUPLING_PLANES for j in range(plan["n"] - 1))


@pytest.mark.parametrize("fmt", ["bf16x3", "f16x2"])
@pytest.mark.parametrize("name", ["synth_d7_k3_soft_ctx", "synth_d7_k3_soft_noctx"])
def test_golden_through_the_emulated_planes_plan_with_a_context(name, fmt, monkeypatch):
    """the reference's soft-training goldens through the planes plan with fused couplings: the plan carries the context launches,
    the base density is reduced in the last GEMM's epilogue, and log_prob / backward / _forward reproduce the reference"""
    emulator.install_prep_emulation(monkeypatch)
    seen = emulator_ctx.install(monkeypatch)
    spec, sd, a = load_case(name)
    flow = build_flow(spec, sd)
    eng = FlowEngine(flow.layers)
    x, zin = a["x"], a["zin"]
    B = x.shape[0]
    ctx = a.get("context")
    lp_ctx = ctx if ctx is not None else torch.zeros(B, 1)           # USFlow.log_prob: soft training without a context = noise level 0
    eng.use_fused_coupling, eng.fused_min_rows = True, 0
    eng.use_planes, eng.planes_min_rows, eng.gemm_mode = True, 0, fmt
    assert eng._planes_ok("backward", B, True, False)
    # log_prob: the planes plan with the base density in the last GEMM's epilogue, as Flow._log_prob_device runs it
    info = flow._base_info(torch.device("cpu"))
    base = _ext.BASE_LAPLACE if info[0] == "laplace" else _ext.BASE_NORMAL
    plan = eng._plan("backward", B, x.device, True, f"base{base}")
    assert plan.get("planes") and plan["has_ctx"] and plan["planes_fmt"] == FMT[fmt]
    assert _has_ctx_launch(plan), "the context coupling launch is not in the planes plan"
    assert plan["n_part"] >= 1, "base density was not reduced in the last GEMM's epilogue"
    ws = plan["ws"]
    emulator._emu_base_tables(base, info[1], info[2], eng.D, ws["btab"], ws["btab"].numel() // 3)
    emulator.run_plan(eng, plan, x.contiguous(), None, lp_ctx)
    assert seen.seen == spec.coupling_blocks
    lp = torch.empty(B)
    emulator._emu_base_logprob(ws["bpart"], 8, B, plan["n_part"], _ext.BASE_ROWSUM, None, None, -float(plan["pk"]["ladj_total"]), lp)
    rel = lambda u, v: ((u.double() - v.double()).abs() / v.double().abs().clamp_min(1e-30)).max().item()      # noqa: E731
    assert rel(lp, a["log_prob64"]) <= 1e-5 and rel(lp, a["log_prob32"]) <= 1e-5
    # backward / _forward: with the fixture's context (the goldens of the fixture without one were made without a context)
    z = emulator.engine_transform(eng, x, "backward", ctx, True, planes=fmt)
    xf = emulator.engine_transform(eng, zin, "forward", ctx, True, planes=fmt)
    if ctx is not None:
        assert len(_ctx_plans(eng)) == 3 and all(_has_ctx_launch(p) for p in _ctx_plans(eng))
    s = max(1.0, a["backward64"].abs().max().item())
    assert (z.double() - a["backward64"]).abs().max().item() < 2e-5 * s
    s = max(1.0, a["forward64"].abs().max().item())
    assert (xf.double() - a["forward64"]).abs().max().item() < 2e-5 * s


def test_context_keeps_the_fp32_plan_where_a_coupling_would_not_run_fused():
    """a context enters the planes pipeline only as the fused launch's start value: three hidden layers in bf16x3, conditioners
    wider than 256 and use_fused_coupling = False keep the fp32-activation plan; without a context they take the planes plan"""
    def eng_of(hidden):
        spec = orc.FlowSpec(40, 2, hidden, householder=0, soft_training=True)
        eng = FlowEngine(build_flow(spec, orc.synth_state_dict(spec, seed=2)).layers)
        eng.use_planes, eng.planes_min_rows, eng.fused_min_rows = True, 0, 0
        return eng
    eng = eng_of([24, 16])
    assert eng._planes_ok("backward", 64, True, False) and eng._planes_ok("forward", 64, True, False)
    eng.use_fused_coupling = False
    assert eng._planes_ok("backward", 64, False, False) and not eng._planes_ok("backward", 64, True, False)
    eng = eng_of([24, 16, 24])
    eng.gemm_mode = "bf16x3"
    assert eng._planes_ok("backward", 64, False, False) and not eng._planes_ok("backward", 64, True, False)
    eng.gemm_mode = "f16x2"
    assert eng._planes_ok("backward", 64, True, False)
    eng._f16_overflow = True                      # the redo of a pass whose range flag fired: bf16x3 planes -> the fp32 plan with the context
    assert not eng._planes_ok("backward", 64, True, False)
    eng = eng_of([300])
    assert eng._planes_ok("backward", 64, False, False) and not eng._planes_ok("backward", 64, True, False)
    eng = eng_of([24, 16])
    eng.fused_min_rows = 1000                     # below the fused kernel's cross-over the couplings are GEMM chains
    assert not eng._planes_ok("backward", 64, True, False) and eng._planes_ok("backward", 1000, True, False)


@pytest.mark.parametrize("hidden,fallbacks", [([24, 16], 1), ([24, 16, 24], 2)])
def test_f16x2_redo_carries_the_context(hidden, fallbacks, monkeypatch):
    """log_prob(x, ctx) in f16x2 whose range flag fires (set here behind every fp16x2 pass): with two hidden layers the redo is
    the bf16x3 planes plan with the context launches and the base density in its epilogue; with three (bf16x3 does not run them
    fused) the redo is no planes plan, latent_base_sums hands the batch back and latent -- whose own fp16x2 pass is void the same
    way -- ends on the fp32-activation plan with the context.  Either way the result is the oracle's"""
    emulator.install_training_emulation(monkeypatch)
    seen = emulator_ctx.install(monkeypatch)
    spec = orc.FlowSpec(40, 2, hidden, householder=0, soft_training=True)
    sd = orc.synth_state_dict(spec, seed=2)
    flow = build_flow(spec, sd)
    eng = flow.engine()
    eng.use_planes, eng.planes_min_rows, eng.fused_min_rows, eng.gemm_mode = True, 0, 0, "f16x2"
    emulated, ran = FlowEngine._execute, []

    def overflowing(self, plan, x, out, context):
        emulated(self, plan, x, out, context)
        ran.append((plan.get("planes_fmt") if plan.get("planes") else None, plan.get("n_part", 0)))
        if plan.get("planes_fmt") == _ext.PLANES_F16X2:
            plan["ws"]["pflag"].fill_(1)
    monkeypatch.setattr(FlowEngine, "_execute", overflowing)
    g = torch.Generator().manual_seed(3)
    x, ctx = torch.rand(50, 40, generator=g), torch.rand(50, 1, generator=g) * 2
    with torch.no_grad():
        lp = flow._log_prob_device(x, ctx)
    assert eng.f16_fallbacks == fallbacks and not eng._f16_overflow
    if len(hidden) == 2:
        assert [r[0] for r in ran] == [_ext.PLANES_F16X2, _ext.PLANES_BF16X3] and ran[1][1] >= 1 and seen.seen == 4
    else:
        assert [r[0] for r in ran] == [_ext.PLANES_F16X2, _ext.PLANES_F16X2, None] and seen.seen == 4
    ref = orc.flow_log_prob(orc.to_dtype(sd, torch.float64), spec, x.double(), ctx.double())
    assert ((lp.double() - ref).abs() / ref.abs()).max().item() <= 1e-5


def test_a_context_takes_the_planes_plans_by_default_only_behind_its_own_row_threshold():
    """automatic mode (use_planes = None) and the training step: a flow with a context keeps the fp32-activation plan / the
    fp32-row path it had, at every batch size, until ctx_planes_min_rows / train_ctx_planes_min_rows name a cross-over; the
    same flow without a context is not touched by either knob"""
    spec = orc.FlowSpec(160, 2, [64, 48], soft_training=True)
    eng = FlowEngine(build_flow(spec, orc.synth_state_dict(spec, seed=2)).layers)
    assert eng.use_planes is None and eng.ctx_planes_min_rows is None and eng.train_ctx_planes_min_rows is None
    for B in (24576, 65536):
        assert eng._planes_ok("backward", B, False, False) and eng._planes_ok("backward", B, False, True)
        assert not eng._planes_ok("backward", B, True, False) and not eng._planes_ok("backward", B, True, True)
    eng.ctx_planes_min_rows = 32768
    assert not eng._planes_ok("backward", 24576, True, False) and eng._planes_ok("backward", 65536, True, False)
    assert not eng._planes_ok("backward", 65536, True, True)
    eng.train_ctx_planes_min_rows = 32768
    assert not eng._planes_ok("backward", 24576, True, True) and eng._planes_ok("backward", 65536, True, True)
    eng.ctx_planes_min_rows = None
    eng.use_planes = True                         # forced, as for every flow
    assert eng._planes_ok("backward", 24576, True, False)


def test_planes_training_with_a_context_matches_oracle_autograd(monkeypatch):
    """the smooth variant (slope 1, Normal base: no kink anywhere) of the planes training step with a context, every entry point
    emulated from its documented semantics: every parameter gradient -- the context layers' layers.1.weight / layers.1.bias
    included -- within 2e-4 of its tensor's largest entry of fp64 autograd through the oracle"""
    from test_training_emulated import oracle_grads
    from usflows_amd import training
    from usflows_amd.training import TrainPath
    emulator.install_training_emulation(monkeypatch)
    seen = emulator_ctx.install(monkeypatch)
    spec = orc.FlowSpec(160, 2, [64, 48], soft_training=True, negative_slope=1.0, base="normal")
    sd = orc.synth_state_dict(spec, seed=9)
    flow = build_flow(spec, sd)
    eng = flow.engine()
    eng.use_planes, eng.planes_min_rows, eng.fused_min_rows, eng.train_planes_min_rows = True, 0, 0, 0
    eng.train_ctx_planes_min_rows = 0
    B = 600
    g = torch.Generator().manual_seed(7)
    x = torch.rand(B, 160, generator=g)
    ctx = torch.rand(B, 1, generator=g) * 2
    g_lp = -(0.5 + torch.rand(B, generator=g)) / B
    path = TrainPath(flow)
    assert path.supported(x, ctx)
    lp = training.log_prob_with_grad(path, x, ctx)
    plan = eng._plan("backward", B, x.device, True, "nat", train=True)
    assert plan.get("planes_train") and plan["has_ctx"] and _has_ctx_launch(plan)
    assert seen.seen == 2
    (lp * g_lp).sum().backward()
    lp_ref, g_ref = oracle_grads(spec, sd, x, g_lp, ctx)
    assert ((lp.detach().double() - lp_ref).abs() / lp_ref.abs()).max().item() <= 1e-5
    checked = []
    for pname, p in flow.named_parameters():
        ref = g_ref.get(pname)
        if not p.requires_grad or ref is None:
            continue
        assert ref.abs().max().item() > 0 and p.grad is not None, pname
        err = (p.grad.double() - ref.reshape(p.shape)).abs().max().item()
        assert err <= 2e-4 * ref.abs().max().item(), (pname, err, ref.abs().max().item())
        checked.append(pname)
    assert sum(".layers.1." in n for n in checked) == 4, checked          # weight and bias of both context layers


def _desc(act=_ext.ACT_LEAKY_RELU):
    """a descriptor that passes usf_coupling_planes' own checks (the pointers are never read: validation comes before any launch)"""
    d = _ext.CouplingPlanesDesc()
    d.z, d.z_nkb, d.M = 0x100000, 4, 40
    d.kb_p0, d.nk_p, d.kb_t0, d.nk_t = 2, 2, 0, 2
    d.n_hidden, d.hidden_padded = 1, 256
    d.W_in, d.ldw_in, d.w_in_plane, d.b_in = 0x200000, 64, 256 * 64, 0x300000
    d.W_out, d.ldw_out, d.w_out_plane, d.b_out = 0x400000, 256, 64 * 256, 0x500000
    d.sign, d.slope, d.act, d.format = 1.0, 0.01, act, _ext.PLANES_BF16X3
    if act == _ext.ACT_GATE:
        d.hidden_out[0], d.gate[0] = 0x600000, 0x700000
    return d


@pytest.mark.parametrize("what,kw,msg", [
    ("gate", dict(act=_ext.ACT_GATE), b"USF_ACT_GATE"),
    ("misaligned w_ctx", dict(w_ctx=0x900004), b"16-byte aligned"),
    ("null b_ctx", dict(b_ctx=None), b"16-byte aligned"),
    ("stride 2", dict(stride=2), b"ctx_stride"),
    ("stride -1", dict(stride=-1), b"ctx_stride"),
])
def test_context_argument_errors_are_reported_without_a_gpu(what, kw, msg):
    lib = _ext.load()
    d = _desc(kw.get("act", _ext.ACT_LEAKY_RELU))
    rc = lib.usf_coupling_planes_ctx(ctypes.byref(d), 0x800000, kw.get("stride", 1), kw.get("w_ctx", 0x900000),
                                     kw.get("b_ctx", 0xA00000), None)
    assert rc < 0 and msg in lib.usf_last_error(), (what, rc, lib.usf_last_error())


def test_context_prefix_op_needs_its_coupling_op():
    """inside an op list the context arguments ride in a USF_OP_CALL op that applies to the USF_OP_COUPLING_PLANES op behind it:
    a list that ends behind the prefix, or continues with another kind of op, is rejected before anything is launched"""
    lib = _ext.load()
    vec = torch.zeros(256)
    arr = (_ext.Op * 2)()
    arr[0] = _ext.coupling_planes_ctx_prefix(vec, 1, vec, vec)
    assert _ext.is_ctx_prefix(arr[0]) and not _ext.is_ctx_prefix(arr[1])
    assert lib.usf_run_ops(arr, 1, None) < 0 and b"USF_FN_COUPLING_PLANES_CTX" in lib.usf_last_error()
    arr[1].kind = _ext.OP_GEMM_PLANES
    assert lib.usf_run_ops(arr, 2, None) < 0 and b"USF_FN_COUPLING_PLANES_CTX" in lib.usf_last_error()
    # a misaligned context vector inside a list: the same check as the direct call
    arr[0].u.call.a[2] = vec.data_ptr() + 4
    arr[1].kind = _ext.OP_COUPLING_PLANES
    arr[1].u.coupling_planes = _desc()
    assert lib.usf_run_ops(arr, 2, None) < 0 and b"16-byte aligned" in lib.usf_last_error()
