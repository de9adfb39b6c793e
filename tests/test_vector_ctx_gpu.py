"""Vector contexts (ConditionalDenseNN with 2 <= context_dim <= 32) on a real MI355X: usf_coupling_additive_vctx_f32 in its three
kernel families against fp64 torch, one coupling layer at a time through the binding; whole flows -- log_prob, backward, _forward,
sample -- against the real reference's fixtures (tests/golden/vctx) on the fused and the unfused plan with no composite fall-back;
and the training path's gradients against the reference's fp64 autograd.  Bounds: those tests/test_flow_gpu.py::test_golden_parity
and tests/test_training_gpu.py apply to the existing scalar-context fixture."""
import warnings

import pytest
import torch

import vctx_cases as vc
from oracle import usflows_oracle as orc
from usflows_amd import _ext as ext
from usflows_amd.synth import build_usflow, synth_state_dict

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
RTOL = 1e-5                 # test_golden_parity: log_prob, relative
ATOL_T = 2e-5               # test_golden_parity: backward / _forward, times max(1, largest reference entry)
GTOL = 2e-4                 # test_training_gpu.py: gradients, of each tensor's largest entry


def _rel(a, b):
    return ((a.double().cpu() - b.double()).abs() / b.double().abs()).max().item()


def _close_t(got, ref):
    s = max(1.0, ref.abs().max().item())
    err = (got.double().cpu() - ref.double().cpu()).abs().max().item()
    print(f"    transform err {err:.3e} (bound {ATOL_T * s:.3e})")
    return err < ATOL_T * s


# ---- kernel level ----------------------------------------------------------------------------------------------------------------
# (kernel expected, rows, D, hidden, C): halves 4 / 3, 17 / 16, 32 / 32
KERNELS = [(3, 37, 7, [16, 16], 3), (1, 300, 33, [40, 24], 5), (2, 1100, 64, [160, 160], 2), (2, 1100, 64, [160, 160], 10),
           (2, 1100, 64, [160, 160], 32)]


@pytest.fixture(scope="module")
def layers():
    """per kernel case: a two-coupling flow's engine (its packers build the padded weight images) and its raw parameters"""
    out = {}
    for variant, M, D, hidden, C in KERNELS:
        spec = orc.FlowSpec(dim=D, coupling_blocks=2, hidden_dims=hidden, householder=0, extra={"context_dim": C})
        sd = synth_state_dict(spec, seed=100 + C)
        flow = build_usflow(spec, sd, device=DEV)
        eng = flow.engine()
        assert eng is not None and eng.ctx_dim == C
        eng.fused_min_rows = 0
        out[(M, D, C)] = (eng, eng.pack(torch.device(DEV)))
    return out


def _reference(eng, cp, z, ctx, sign, W_ctx=None):
    """fp64 torch: out[:, trans] = z[:, trans] + sign * MLP(z[:, pass], ctx) on the segment-layout rows z"""
    raw = cp["raw"]
    pi, ti = raw["pass_idx"].long().cpu(), raw["tr_idx"].long().cpu()
    npass, ntr = int((pi >= 0).sum()), int((ti >= 0).sum())
    z = z.double().cpu()
    W, b = (t.double().cpu() for t in raw["first"])
    Wc, bc = (t.double().cpu() for t in raw["ctx"])
    if W_ctx is not None:
        Wc = W_ctx.double().cpu()
    slope = cp["slope"]
    act = lambda v: torch.where(v > 0, v, v * slope)      # noqa: E731
    h = z[:, cp["pass_off"]: cp["pass_off"] + npass] @ W[:, pi[:npass]].t() + b
    h = act(h + (ctx.double().cpu() @ Wc.t() + bc))
    for Wh, bh in raw["hidden"]:
        h = act(h @ Wh.double().cpu().t() + bh.double().cpu())
    Wl, bl = (t.double().cpu() for t in raw["last"])
    out = z.clone()
    out[:, cp["tr_off"]: cp["tr_off"] + ntr] += sign * (h @ Wl[ti[:ntr]].t() + bl[ti[:ntr]])
    return out, ntr


@pytest.mark.parametrize("variant,M,D,hidden,C", KERNELS, ids=[f"k{k[0]}_M{k[1]}_C{k[4]}" for k in KERNELS])
def test_vctx_kernel_vs_fp64(variant, M, D, hidden, C, layers):
    """one coupling layer through the binding, both mask orientations x sign +-1; one context row for all rows (ld_ctx = 0); NaN in
    the workspace's padding columns; and a W_ctx whose columns 1.. are zero against the scalar-context entry on column 0"""
    eng, pk = layers[(M, D, C)]
    g = torch.Generator().manual_seed(M + C)
    Cp = -(-C // 4) * 4
    for i, cp in pk["coupling"].items():
        f = eng._fused_pack(cp)
        Wt, bctx = f["W_ctx_t"], f["b_ctx"]
        assert Wt.shape[0] == C and Wt.shape[1] == f["Hp"]
        z0 = torch.zeros(M, eng.LD)
        real = eng.seg_idx >= 0
        z0[:, real] = torch.rand(M, int(real.sum()), generator=g) * 2 - 1
        ctx = torch.zeros(M, Cp)
        ctx[:, :C] = torch.rand(M, C, generator=g) * 2 - 1
        ctx_d = ctx.to(DEV)

        def launch(z, sign, cbuf, ld, wt=Wt):
            op = eng._coupling_op(cp, z.data_ptr(), M, sign, None)
            assert ext.coupling_vctx_variant(op, C) == variant, (ext.coupling_vctx_variant(op, C), variant)
            ext.coupling_vctx_op(op, cbuf, ld, C, wt, wt.shape[1], bctx, z.device)
            torch.cuda.synchronize()
            return z

        for sign in (1.0, -1.0):
            ref, ntr = _reference(eng, cp, z0, ctx[:, :C], sign)
            cols = slice(0, eng.LD)
            got = launch(z0.to(DEV), sign, ctx_d, Cp)
            assert _close_t(got[:, cols], ref[:, cols]), (i, sign)
            # the padding columns [C, Cp) are loaded but never multiplied in: NaN there changes nothing
            if Cp > C:
                poisoned = ctx_d.clone()
                poisoned[:, C:] = float("nan")
                assert torch.equal(launch(z0.to(DEV), sign, poisoned, Cp), got), (i, sign, "NaN padding")
        # ld_ctx = 0: one row for all rows
        row = ctx_d[5].clone()
        ref, _ = _reference(eng, cp, z0, ctx[5:6, :C].expand(M, C), -1.0)
        got0 = launch(z0.to(DEV), -1.0, row, 0)
        assert _close_t(got0, ref), (i, "ld_ctx 0")
        assert torch.equal(got0, launch(z0.to(DEV), -1.0, row[None].expand(M, Cp).contiguous(), Cp))
        # columns 1.. of W_ctx zero: the scalar-context entry on column 0 computes the same layer
        wt1 = torch.zeros_like(Wt)
        wt1[0] = Wt[0]
        got1 = launch(z0.to(DEV), 1.0, ctx_d, Cp, wt1)
        zs = z0.to(DEV)
        op = eng._coupling_op(cp, zs.data_ptr(), M, 1.0, None)
        c0 = ctx_d[:, 0].contiguous()
        w0 = wt1[0].contiguous()
        op.u.coupling.context, op.u.coupling.W_ctx, op.u.coupling.b_ctx = c0.data_ptr(), w0.data_ptr(), bctx.data_ptr()
        assert ext.load().usf_coupling_variant(op.u.coupling) == variant
        ext.coupling_op(op, zs.device)
        torch.cuda.synchronize()
        assert _close_t(got1, zs), (i, "scalar entry")
        # ctx == NULL is exactly usf_coupling_additive_f32
        za, zb = z0.to(DEV), z0.to(DEV)
        ext.coupling_vctx_op(eng._coupling_op(cp, za.data_ptr(), M, 1.0, None), None, 0, 0, None, 0, None, za.device)
        ext.coupling_op(eng._coupling_op(cp, zb.data_ptr(), M, 1.0, None), zb.device)
        torch.cuda.synchronize()
        assert torch.equal(za, zb)


# ---- flow level ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def loaded():
    return {n: vc.load(n) for n in vc.CASES}


def _rows(name, t):
    return t if vc.CASES[name][5] else t[vc.kept_rows(vc.CASES[name][2]).to(t.device)]


@pytest.mark.parametrize("fused", [True, False])
@pytest.mark.parametrize("name", list(vc.CASES))
def test_flow_parity_with_the_reference(name, fused, loaded):
    spec, sd, a, _ = loaded[name]
    x, zin, ctx = (t.to(DEV) for t in vc.inputs(name))
    C, n = vc.CASES[name][1], vc.CASES[name][2]
    flow = vc.build(name, sd, device=DEV)
    eng = flow.engine()
    assert eng is not None and eng.ctx_dim == C
    eng.use_fused_coupling, eng.fused_min_rows = fused, 0
    n0 = eng.launch_count
    with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)            # no composite fall-back
        with torch.no_grad():
            lp = flow.log_prob(x, ctx)
            z = flow.backward(x, ctx)
            xf = flow._forward(zin, ctx)
            torch.cuda.synchronize()
            assert eng.launch_count > n0, "HIP path did not run"
            print(f"  {name} fused={fused}: log_prob rel err vs fp64 {_rel(lp, a['log_prob64']):.3e}, vs fp32 {_rel(lp, a['log_prob32']):.3e}")
            assert _rel(lp, a["log_prob64"]) < RTOL and _rel(lp, a["log_prob32"]) < RTOL
            assert _close_t(_rows(name, z), a["backward64"]) and _close_t(_rows(name, xf), a["forward64"])
            # a [C] context is the same row repeated n times, bit for bit
            one = ctx[1].clone()
            rep = one[None].expand(n, C).contiguous()
            assert torch.equal(flow.backward(x, one), flow.backward(x, rep))
            assert torch.equal(flow.log_prob(x, one[None]), flow.log_prob(x, rep))
            # sample = _forward of the same Philox noise with the context
            info = flow._base_info(torch.device(DEV))
            m = 19
            noise = torch.empty(m, eng.D, dtype=torch.float32, device=DEV)
            base = ext.BASE_LAPLACE if info[0] == "laplace" else ext.BASE_NORMAL
            ext.base_sample(noise, eng.D, m, eng.D, base, info[1], info[2], 7, 0, 0)
            xs = flow.sample([m], ctx[:m].contiguous(), seed=7)
            assert torch.equal(xs, flow._forward(noise, ctx[:m].contiguous()))
    n_vctx = sum(1 for p in eng._plans.values() for j in range(p["n"])
                 if p["arr"][j].kind == ext.OP_CALL and p["arr"][j].u.call.fn == ext.FN_COUPLING_VCTX)
    assert (n_vctx > 0) == fused and not any(p.get("planes") for p in eng._plans.values())


# ---- training --------------------------------------------------------------------------------------------------------------------
def _grads(flow, x, ctx):
    for p in flow.parameters():
        p.grad = None
    lp = flow.log_prob(x, ctx)
    assert lp.requires_grad
    (-lp.mean()).backward()
    return lp.detach()


@pytest.mark.parametrize("name", ["d7_k3", "d33_k2", "d64_k2_c10", "d64_k2_c32"])
def test_training_gradients_match_the_reference(name, loaded):
    """37 rows (the tiny-layer kernel's step), 300 (fp32-row path) and 1100 rows (the bf16x3 kernel's saved activations)"""
    spec, sd, a, g_ref = loaded[name]
    x, _, ctx = (t.to(DEV) for t in vc.inputs(name))
    flow = vc.build(name, sd, device=DEV)
    eng = flow.engine()
    n0 = eng.launch_count
    with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)
        lp = _grads(flow, x, ctx)
    torch.cuda.synchronize()
    assert eng.launch_count > n0, "device training path did not run"
    assert _rel(lp, a["log_prob64"]) < RTOL
    named = dict(flow.named_parameters())
    worst = 0.0
    for k, ref in g_ref.items():
        got = named[k].grad
        assert got is not None and got.shape == ref.shape, k
        big = ref.abs().max().item()
        err = (got.double().cpu() - ref).abs().max().item()
        worst = max(worst, err / big)
        assert err <= GTOL * big, (k, err, big)
    print(f"  {name}: worst gradient error {worst:.3e} of a tensor's largest entry (bound {GTOL:.0e})")
    assert any(k.endswith("layers.1.weight") for k in g_ref)


@pytest.mark.parametrize("dim,hidden,C,rows", vc.WIDE, ids=[f"h{w[1][0]}_C{w[2]}_M{w[3]}" for w in vc.WIDE])
def test_training_gradients_with_a_context_wider_than_the_hidden_layers(dim, hidden, C, rows):
    """Cp = round_up(C, 4) above the widest hidden layer and the row width (the context layer's gradient image is sized by Cp),
    at a batch whose weight gradients are queued jobs (37 rows) and one where they are direct launches (300), against autograd
    through the fp64 oracle"""
    spec, sd, x, ctx, g_ref, lp_ref = vc.wide_case(dim, hidden, C, rows)
    flow = build_usflow(spec, sd, device=DEV)
    eng = flow.engine()
    assert -(-C // 4) * 4 > max(eng.hmax, eng.LD)
    n0 = eng.launch_count
    with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)
        lp = _grads(flow, x.to(DEV), ctx.to(DEV))
    torch.cuda.synchronize()
    assert eng.launch_count > n0 and _rel(lp, lp_ref) < RTOL
    named = dict(flow.named_parameters())
    worst, checked = 0.0, 0
    for k, ref in g_ref.items():
        if k not in named or not named[k].requires_grad:
            continue
        got, big = named[k].grad, ref.abs().max().item()
        assert got is not None and got.shape == ref.shape, k
        err = (got.double().cpu() - ref).abs().max().item()
        worst = max(worst, err / big)
        assert err <= GTOL * big, (k, err, big)
        checked += 1
    print(f"  wide h{hidden} C{C} M{rows}: worst gradient error {worst:.3e} (bound {GTOL:.0e})")
    assert checked >= 10 and named["trainable_layers.1.conditioner.layers.1.weight"].grad.shape == (hidden[0], C)


def test_an_optimiser_step_replays_to_the_same_bits(loaded):
    """the same SGD step from the same parameters, once on a fresh workspace and once after passes with OTHER contexts (rows, one
    broadcast row) through the same workspace: nothing stale stays in the context columns"""
    name = "d7_k3"
    spec, sd, a, _ = loaded[name]
    x, _, ctx = (t.to(DEV) for t in vc.inputs(name))
    flow = vc.build(name, sd, device=DEV)
    sd0 = {k: v.detach().clone() for k, v in flow.state_dict().items()}

    def step():
        opt = torch.optim.SGD(flow.parameters(), lr=1e-2)
        _grads(flow, x, ctx)
        opt.step()
        torch.cuda.synchronize()
        return {k: v.detach().clone() for k, v in flow.state_dict().items()}

    first = step()
    flow.load_state_dict(sd0)
    other = torch.rand_like(ctx) * 3 + 1
    _grads(flow, x, other)
    with torch.no_grad():
        flow.log_prob(x, other[2])
        flow.log_prob(x, other)
    second = step()
    assert all(torch.equal(first[k], second[k]) for k in first)
    assert any(not torch.equal(first[k], sd0[k]) for k in first)
    # a SECOND step, from the updated parameters: the packed images (the transposed W_ctx among them) must follow the update --
    # against the torch composite on a CPU copy of the updated flow
    lp_dev = _grads(flow, x, ctx)
    torch.cuda.synchronize()
    cpu = vc.build(name, {k: v.cpu() for k, v in second.items()})
    lp_cpu = cpu.log_prob(x.cpu(), ctx.cpu())
    (-lp_cpu.mean()).backward()
    assert _rel(lp_dev, lp_cpu.detach()) < RTOL
    dev_named, moved = dict(flow.named_parameters()), 0
    for k, p in cpu.named_parameters():
        if p.grad is None:
            continue
        big = p.grad.abs().max().item()
        assert (dev_named[k].grad.cpu().double() - p.grad.double()).abs().max().item() <= GTOL * big, k
        moved += 1
    assert moved >= 20
    # (and the step did move the context weights: a stale image would have kept the first step's values)
    wk = "trainable_layers.1.conditioner.layers.1.weight"
    assert not torch.equal(second[wk], sd0[wk])
