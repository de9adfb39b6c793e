"""Vector contexts (ConditionalDenseNN with 2 <= context_dim <= 32) on the host side, no GPU: the composite mirror and the fp64
oracle against the real reference's fixtures (tests/golden/vctx, tests/golden/make_golden_vector_ctx.py); the engine's fused and
unfused plans and the training path interpreted on the CPU (tests/emulator_vctx.py restates usf_coupling_additive_vctx_f32 and its
prefix op); which flows the engine accepts; the ABI of the new entry points and their argument checks, which run before any
launch; and the synthetic generator's draws for existing specs."""
import ctypes
import os
import re
import warnings

import pytest
import torch

import emulator
import emulator_vctx
import vctx_cases as vc
from golden_util import load_case
from oracle import usflows_oracle as orc
from usflows_amd import _ext
from usflows_amd.engine import FlowEngine

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RTOL = 1e-5            # tests/test_flow_gpu.py::test_golden_parity's bound on log_prob (the existing context fixture's)


def _rel(a, b):
    return ((a.double() - b.double()).abs() / b.double().abs()).max().item()


def _rows(name, t):
    """the rows a fixture keeps of a transform's result"""
    return t if vc.CASES[name][5] else t[vc.kept_rows(vc.CASES[name][2])]


@pytest.fixture(scope="module")
def loaded():
    return {n: vc.load(n) for n in vc.CASES}


# ---- composite parity ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(vc.CASES))
def test_composite_mirror_and_oracle_reproduce_the_reference(name, loaded):
    """the torch mirror on the CPU (the composite path) and the fp64 oracle handed the same state dict, against the fixture"""
    spec, sd, a, _ = loaded[name]
    assert float(a["ref_gap"]) < RTOL            # the reference's own fp32-vs-fp64 gap on these inputs stays inside the bound
    x, zin, ctx = vc.inputs(name)
    flow = vc.build(name, sd)
    with torch.no_grad():
        lp = flow.log_prob(x, ctx)
        z = flow.backward(x, ctx)
        xf = flow._forward(zin, ctx)
    assert _rel(lp, a["log_prob64"]) < RTOL and _rel(lp, a["log_prob32"]) < RTOL
    for got, key in ((z, "backward64"), (xf, "forward64")):
        s = max(1.0, a[key].abs().max().item())
        assert (_rows(name, got).double() - a[key]).abs().max().item() < 2e-5 * s, key
    lp64 = orc.flow_log_prob(orc.to_dtype(sd, torch.float64), spec, x.double(), ctx.double())
    assert _rel(lp64, a["log_prob64"]) < 1e-12


# ---- emulated plans -----------------------------------------------------------------------------------------------------
def _vctx_launches(plan):
    arr = plan["arr"]
    return sum(1 for j in range(plan["n"] - 1) if arr[j].kind == _ext.OP_CALL and arr[j].u.call.fn == _ext.FN_COUPLING_VCTX
               and arr[j + 1].kind == _ext.OP_COUPLING)


@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("name", vc.SMALL)
def test_engine_plans_reproduce_the_fixtures(name, fused, loaded, monkeypatch):
    """the engine's fused (prefix op + coupling op = one usf_coupling_additive_vctx_f32 launch) and unfused (context GEMM at
    K = Cp) plans, both directions and the log_prob path, in fp64 arithmetic"""
    emulator.install_training_emulation(monkeypatch)
    seen = emulator_vctx.install(monkeypatch)
    spec, sd, a, _ = loaded[name]
    x, zin, ctx = vc.inputs(name)
    flow = vc.build(name, sd)
    eng = FlowEngine(flow.layers)
    C = vc.CASES[name][1]
    assert eng.ctx_dim == C
    eng.use_fused_coupling, eng.fused_min_rows, eng.use_planes, eng.use_graphs = fused, 0, True, False
    z = eng.transform(x, "backward", ctx)
    xf = eng.transform(zin, "forward", ctx)
    for got, key in ((z, "backward64"), (xf, "forward64")):
        s = max(1.0, a[key].abs().max().item())
        assert (got.double() - a[key]).abs().max().item() < 2e-5 * s, key
    zbuf, ldz, logdet = eng.latent(x, ctx)
    lp = orc.base_log_prob(spec, zbuf[:, : eng.D].double(), orc.to_dtype(sd, torch.float64)) - float(logdet)
    assert _rel(lp, a["log_prob64"]) < RTOL
    plans = list(eng._plans.values())
    assert plans and not any(p.get("planes") for p in plans)             # a vector context never takes the planes plans
    n_cpl = sum(1 for s_ in eng.steps if s_.kind == "coupling")
    if fused:
        assert all(_vctx_launches(p) == n_cpl for p in plans) and seen.seen == 3 * n_cpl
    else:
        assert not any(_vctx_launches(p) for p in plans) and seen.seen == 0
        Cp = -(-C // 4) * 4
        assert plans[0]["ws"]["ctx4"].shape == (x.shape[0], Cp)
        assert any(p["arr"][j].kind == _ext.OP_LINEAR and p["arr"][j].u.linear.K == Cp and p["arr"][j].u.linear.lda == Cp
                   for p in plans for j in range(p["n"]))
    # one row for all rows: [C] and [1, C] are the row repeated
    one = ctx[3]
    want = eng.transform(x, "backward", one.expand(x.shape[0], C).contiguous())
    assert torch.equal(eng.transform(x, "backward", one), want) and torch.equal(eng.transform(x, "backward", one[None].double()), want)
    with pytest.raises(ValueError):
        eng.transform(x, "backward", torch.zeros(x.shape[0]))            # a 1-D [n] context: an error in the reference too


@pytest.mark.parametrize("name", vc.SMALL)
def test_training_path_reproduces_the_fixture_gradients(name, loaded, monkeypatch):
    """forward + hand-derived backward (tiny-kernel step at <= 256 rows, fp32-row path above), every parameter's gradient --
    layers[1].weight [h0, C] and layers[1].bias included -- against the reference's fp64 autograd"""
    from usflows_amd import training
    from usflows_amd.training import TrainPath
    emulator.install_training_emulation(monkeypatch)
    seen = emulator_vctx.install(monkeypatch)
    spec, sd, a, g_ref = loaded[name]
    x, _, ctx = vc.inputs(name)
    flow = vc.build(name, sd)
    path = TrainPath(flow)
    assert path.supported(x, ctx) and not path.supported(x, ctx.clone().requires_grad_(True))
    lp = training.log_prob_with_grad(path, x, ctx)
    (-lp.mean()).backward()
    assert _rel(lp.detach(), a["log_prob64"]) < RTOL
    named = dict(flow.named_parameters())
    checked = 0
    for k, ref in g_ref.items():
        got = named[k].grad
        assert got is not None and got.shape == ref.shape, k
        big = ref.abs().max().item()
        assert (got.double() - ref).abs().max().item() <= 2e-4 * big, (k, (got.double() - ref).abs().max().item(), big)
        checked += 1
    C = vc.CASES[name][1]
    assert checked >= 20 and any(k.endswith("layers.1.weight") and v.shape[1] == C for k, v in g_ref.items())
    if x.shape[0] <= 256:
        assert seen.seen > 0                      # the tiny-layer kernel's training step took the vector context


@pytest.mark.parametrize("dim,hidden,C,rows", vc.WIDE, ids=[f"h{w[1][0]}_C{w[2]}_M{w[3]}" for w in vc.WIDE])
def test_training_path_with_a_context_wider_than_the_hidden_layers(dim, hidden, C, rows, monkeypatch):
    """Cp = round_up(C, 4) above the widest hidden layer and the row width: the gradient image of layers[1].weight is sized by Cp
    (the emulated weight gradient refuses a view that does not fit its buffer), at a queued-job batch and above it"""
    from usflows_amd import training
    from usflows_amd.synth import build_usflow
    from usflows_amd.training import TrainPath
    emulator.install_training_emulation(monkeypatch)
    emulator_vctx.install(monkeypatch)
    spec, sd, x, ctx, g_ref, lp_ref = vc.wide_case(dim, hidden, C, rows)
    flow = build_usflow(spec, sd)
    eng = flow.engine()
    assert -(-C // 4) * 4 > max(eng.hmax, eng.LD)
    path = TrainPath(flow)
    assert path.supported(x, ctx)
    lp = training.log_prob_with_grad(path, x, ctx)
    (-lp.mean()).backward()
    assert _rel(lp.detach(), lp_ref) < RTOL
    named = dict(flow.named_parameters())
    checked = 0
    for k, ref in g_ref.items():
        if k not in named or not named[k].requires_grad:
            continue                       # (the inverse blocks' aliases of one tensor)
        got, big = named[k].grad, ref.abs().max().item()
        assert got is not None and got.shape == ref.shape, k
        assert (got.double() - ref).abs().max().item() <= 2e-4 * big, (k, (got.double() - ref).abs().max().item(), big)
        checked += 1
    assert checked >= 10 and named["trainable_layers.1.conditioner.layers.1.weight"].grad.shape == (hidden[0], C)


# ---- which flows the engine takes ------------------------------------------------------------------------------------------
def _flow(C, dim=8, blocks=2):
    spec = orc.FlowSpec(dim=dim, coupling_blocks=blocks, hidden_dims=[16], householder=0, extra={"context_dim": C})
    from usflows_amd.synth import build_usflow
    return build_usflow(spec, None)


@pytest.mark.parametrize("C", [2, 3, 10, 32])
def test_engine_accepts_context_widths_up_to_32(C):
    with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)
        eng = _flow(C).engine()
    assert eng is not None and eng.ctx_dim == C


def test_engine_rejects_wider_and_mixed_contexts():
    assert _flow(33).engine() is None
    flow = _flow(3)
    from usflows_amd.networks import ConditionalDenseNN
    cpl = [l for l in flow.layers if type(l).__name__ == "MaskedCoupling"]
    cpl[1].conditioner = ConditionalDenseNN(8, 5, [16], 8, torch.nn.LeakyReLU(0.01))
    assert flow.engine() is None
    assert _flow(1).engine().ctx_dim == 1


# ---- ABI ------------------------------------------------------------------------------------------------------------------
def test_abi_of_the_new_entry_points():
    hdr = open(os.path.join(ROOT, "include", "usflows_hip_internal.h")).read()
    pub = open(os.path.join(ROOT, "include", "usflows_hip.h")).read()
    lib = _ext.load()
    assert int(re.search(r"^#define USF_INTERNAL_VERSION (\d+)", hdr, flags=re.M).group(1)) == _ext.USF_INTERNAL_VERSION == 6
    assert lib.usf_internal_version() == 6
    assert int(re.search(r"^#define USF_ABI_VERSION (\d+)", pub, flags=re.M).group(1)) == _ext.USF_ABI_VERSION == lib.usf_abi_version() == 36
    for name in ("usf_coupling_additive_vctx_f32", "usf_coupling_additive_vctx_variant"):
        assert re.search(rf"\b{name}\s*\(", hdr) and name in _ext.INTERNAL_SYMBOLS and name not in pub and hasattr(lib, name)
    assert int(re.search(r"^#define USF_FN_COUPLING_VCTX (\d+)", hdr, flags=re.M).group(1)) == _ext.FN_COUPLING_VCTX
    assert int(re.search(r"^#define USF_VCTX_MAX (\d+)", hdr, flags=re.M).group(1)) == _ext.VCTX_MAX == 32
    assert _ext.FN_COUPLING_VCTX >= 64 and _ext.FN_COUPLING_VCTX != _ext.FN_COUPLING_PLANES_CTX


def _desc(M=300, n_pass=20, hidden=(40, 24), n_trans=16):
    d = _ext.CouplingDesc()
    d.z = d.out = 0x100000
    d.ldz = d.ldo = 64
    d.M, d.off_pass, d.n_pass, d.off_trans, d.n_trans = M, 20, n_pass, 0, n_trans
    d.n_hidden = len(hidden)
    for i, h in enumerate(hidden):
        d.hidden[i] = h
    d.W_in, d.ldw_in, d.b_in = 0x200000, 32, 0x300000
    for i in range(1, len(hidden)):
        d.W_hid[i - 1], d.ldw_hid[i - 1], d.b_hid[i - 1] = 0x400000 + 0x10000 * i, 64, 0x300000
    d.W_out, d.ldw_out, d.b_out = 0x800000, 64, 0x300000
    d.sign, d.slope, d.act = 1.0, 0.01, _ext.ACT_LEAKY_RELU
    return d


def _call(d, ctx=0x900000, ld=8, C=5, w=0xa00000, ldw=64, b=0xb00000):
    lib = _ext.load()
    return lib.usf_coupling_additive_vctx_f32(ctypes.byref(d), ctx, ld, C, w, ldw, b, None), lib.usf_last_error()


def test_arguments_are_checked_before_any_launch():
    """every rejection below returns before a kernel is launched (there is no GPU here, and the pointers are made up)"""
    for kw, msg in ((dict(C=0), b"ctx_dim"), (dict(C=33), b"ctx_dim"), (dict(ctx=0x900004), b"aligned"), (dict(w=0xa00008), b"aligned"),
                    (dict(b=0xb00004), b"aligned"), (dict(ld=6), b"ld_ctx"), (dict(ld=4), b"ld_ctx"), (dict(ldw=62), b"ldw_ctx"),
                    (dict(ldw=32), b"ldw_ctx"), (dict(w=0), b"W_ctx_t")):
        rc, err = _call(_desc(), **kw)
        assert rc < 0 and msg in err, (kw, rc, err)
    d = _desc()
    d.act = _ext.ACT_GATE
    rc, err = _call(d)
    assert rc < 0 and b"USF_ACT_GATE" in err
    d = _desc()
    d.context = 0x900000
    rc, err = _call(d)
    assert rc < 0 and b"must be NULL" in err
    # the prefix op needs its six arguments and a coupling op behind it
    vec = torch.zeros(64)
    arr = (_ext.Op * 2)()
    arr[0] = _ext.coupling_vctx_prefix(vec, 8, 5, vec, 64, vec)
    arr[1].kind = _ext.OP_LINEAR
    lib = _ext.load()
    assert _ext.is_ctx_prefix(arr[0]) and not _ext.is_ctx_prefix(arr[1])
    assert lib.usf_run_ops(arr, 1, None) < 0 and b"USF_FN_COUPLING_VCTX" in lib.usf_last_error()
    assert lib.usf_run_ops(arr, 2, None) < 0 and b"USF_FN_COUPLING_VCTX" in lib.usf_last_error()


def test_variant_query_counts_the_context_against_the_tiny_kernels_lds():
    """the kernel the entry point would run: the tiny-layer kernel while the layer's images and the context segments fit 64 KB of
    LDS, another kernel (not an error) when they no longer do; ctx_dim 0 is usf_coupling_variant"""
    lib = _ext.load()
    variant = lambda d, C: lib.usf_coupling_additive_vctx_variant(ctypes.byref(d), C)      # noqa: E731
    tiny = _desc(M=37, n_pass=4, hidden=(16, 16), n_trans=3)
    tiny.off_pass, tiny.off_trans = 4, 0
    assert variant(tiny, 0) == lib.usf_coupling_variant(ctypes.byref(tiny)) == 3 and variant(tiny, 3) == 3 and variant(tiny, 32) == 3
    assert variant(_desc(), 5) == 1 and variant(_desc(M=37, n_pass=20, hidden=(40, 24)), 5) == 3
    # a layer near the budget (58.7 KB of the 64 KB without a context): 8 columns still fit, 32 (+ 7.8 KB) do not -- the MFMA kernel
    edge = _desc(M=256, n_pass=52, hidden=(32, 32), n_trans=48)
    edge.off_pass, edge.off_trans, edge.ldz, edge.ldo, edge.ldw_in = 48, 0, 100, 100, 64
    assert [variant(edge, C) for C in (0, 1, 8, 32)] == [3, 3, 3, 1]


# ---- the synthetic generator ------------------------------------------------------------------------------------------------
def test_synthetic_parameters_of_existing_specs_are_unchanged():
    """ModelSpec.extra["context_dim"] defaults to 1 and changes no random draw: a spec without it regenerates an existing fixture's
    stored parameters bit for bit, and the oracle's twin generator still agrees"""
    from usflows_amd.synth import synth_state_dict
    for name in ("synth_d7_k3_soft_ctx", "synth_d16_k4_hh2_conj_laplace"):
        spec, sd, _ = load_case(name)
        assert "context_dim" not in spec.extra
        import numpy as np
        z = np.load(os.path.join(ROOT, "tests", "golden", name + ".npz"), allow_pickle=False)
        mine = synth_state_dict(spec, seed=int(z["seed"]), alpha=float(z["alpha"]))
        twin = orc.synth_state_dict(spec, seed=int(z["seed"]), alpha=float(z["alpha"]))
        assert set(mine) == set(twin)
        n = 0
        for k, v in mine.items():
            assert torch.equal(v, twin[k]), k
            if k in sd:
                assert torch.equal(v, sd[k]), k
                n += 1
        assert n >= 10
    wide = synth_state_dict(vc.spec_of("d16_k3"), seed=1)
    assert wide["trainable_layers.1.conditioner.layers.1.weight"].shape == (32, 10)
