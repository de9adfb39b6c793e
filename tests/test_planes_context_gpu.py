"""A context on the planes pipeline, on a real MI355X: usf_coupling_planes_ctx (the fused planes coupling whose first layer starts at
b_in + b_ctx + ctx * w_ctx: ConditionalDenseNN with context_dim 1, networks.py:739-751) against fp64 arithmetic, and conditional /
soft-trained flat flows through the planes plans -- log_prob, backward, _forward, sample and the training step -- against the
reference's goldens, the fp64 oracle and the fp32-activation / fp32-row paths."""
import math
import warnings

import pytest
import torch

import emulator
from golden_util import load_case
from model_util import build_flow
from oracle import usflows_oracle as orc
from test_planes_gpu import _view, _weight_planes

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FMT = {"bf16x3": 0, "f16x2": 1}


def _ext():
    from usflows_amd import _ext
    _ext.load()
    return _ext


def _force_planes(eng, fmt="bf16x3"):
    eng.gemm_mode = fmt
    eng.use_planes, eng.planes_min_rows, eng.fused_min_rows, eng.train_planes_min_rows = True, 0, 0, 0
    eng.train_ctx_planes_min_rows = 0


def _has_ctx_launch(plan):
    ext = _ext()
    arr = plan["arr"]
    return any(ext.is_ctx_prefix(arr[j]) and arr[j + 1].kind == ext.OP_COUPLING_PLANES for j in range(plan["n"] - 1))


def _ctx_plans(eng):
    return [p for p in eng._plans.values() if p.get("planes") and p.get("has_ctx")]


# ---- 1. the kernel ---------------------------------------------------------------------------------------------------------------
def _decoded_weight(Wp):
    """logical fp32 matrix a weight-planes image holds (the sum of its planes, K axis back in logical order)"""
    W = Wp[0].float() + Wp[1].float() + (Wp[2].float() if Wp.shape[0] == 3 else 0)
    K = W.shape[1]
    slot = torch.tensor([32 * (c // 32) + emulator._SLOT_OF_FEATURE[c % 32] for c in range(K)])
    return W[:, slot]


def _pad_rows(buf, M, nkb, fmt):
    """the planes entries of the last panel's rows >= M (line 16 g + j of a chunk holds row j of the panel)"""
    v = _view(buf, M, nkb, fmt)
    return v[-1].reshape(nkb, v.shape[2], 4, 16, 8)[:, :, :, M - 16 * (v.shape[0] - 1):]


def _batch_rows_equal(a, b, M, nkb, fmt):
    """the planes entries of rows < M, byte for byte"""
    va, vb = _view(a, M, nkb, fmt), _view(b, M, nkb, fmt)
    r0 = M - 16 * (va.shape[0] - 1)
    last = lambda v: v[-1].reshape(nkb, v.shape[2], 4, 16, 8)[:, :, :, :r0]      # noqa: E731
    return torch.equal(va[:-1], vb[:-1]) and torch.equal(last(va), last(vb))


class _Layer:
    """one coupling layer's operands: conditioning blocks [nk_t, nk_t + nk_p), transformed blocks [0, nk_t), hidden widths
    200 / 136 / 72 padded to 256"""

    def __init__(self, ext, fmt, nh, nk_p, nk_t, seed):
        g = torch.Generator().manual_seed(seed)
        self.ext, self.f, self.nh, self.nk_p, self.nk_t = ext, FMT[fmt], nh, nk_p, nk_t
        self.nkb = nk_p + nk_t
        widths = [200, 136, 72][:nh]
        pad = lambda W, r, c: torch.nn.functional.pad(W, (0, c - W.shape[1], 0, r - W.shape[0]))      # noqa: E731
        padv = lambda b, n: torch.nn.functional.pad(b, (0, n - b.numel()))                            # noqa: E731
        k_in = 32 * nk_p
        mats = [pad(torch.randn(widths[0], k_in, generator=g) / math.sqrt(k_in), 256, k_in)]
        for j in range(1, nh):
            mats.append(pad(torch.randn(widths[j], widths[j - 1], generator=g) / math.sqrt(widths[j - 1]), 256, 256))
        mats.append(pad(torch.randn(32 * nk_t, widths[-1], generator=g) / math.sqrt(widths[-1]), 32 * nk_t, 256))
        self.b = [padv(torch.randn(w, generator=g) * 0.1, 256) for w in widths] + [torch.randn(32 * nk_t, generator=g) * 0.1]
        self.w_ctx = padv(torch.randn(widths[0], generator=g) * 0.5, 256)
        self.b_ctx = padv(torch.randn(widths[0], generator=g) * 0.1, 256)
        planes = [_weight_planes(W, W.shape[0], self.f) for W in mats]
        self.W = [_decoded_weight(P) for P in planes]            # what the kernel multiplies (fp16x2: 22 significant bits)
        self.dev = dict(W=[P.to(DEV) for P in planes], b=[b.to(DEV) for b in self.b], w_ctx=self.w_ctx.to(DEV),
                        b_ctx=self.b_ctx.to(DEV), zeros=torch.zeros(256, device=DEV))
        self.flag = torch.zeros(1, dtype=torch.int32, device=DEV)

    def op(self, z, M, sign, hidden_out=None):
        ext, d_ = self.ext, self.dev
        op = ext.Op()
        op.kind = ext.OP_COUPLING_PLANES
        d = op.u.coupling_planes
        d.z, d.z_nkb, d.M = z.data_ptr(), self.nkb, M
        d.kb_p0, d.nk_p, d.kb_t0, d.nk_t = self.nk_t, self.nk_p, 0, self.nk_t
        d.n_hidden, d.hidden_padded = self.nh, 256
        Wi = d_["W"][0]
        d.W_in, d.ldw_in, d.w_in_plane, d.b_in = Wi.data_ptr(), Wi.shape[2], Wi.shape[1] * Wi.shape[2], d_["b"][0].data_ptr()
        for j in range(1, self.nh):
            Wh = d_["W"][j]
            d.W_hid[j - 1], d.b_hid[j - 1] = Wh.data_ptr(), d_["b"][j].data_ptr()
            d.ldw_hid, d.w_hid_plane = Wh.shape[2], Wh.shape[1] * Wh.shape[2]
        Wo = d_["W"][-1]
        d.W_out, d.ldw_out, d.w_out_plane, d.b_out = Wo.data_ptr(), Wo.shape[2], Wo.shape[1] * Wo.shape[2], d_["b"][-1].data_ptr()
        d.sign, d.slope, d.act, d.format, d.range_flag = sign, 0.01, ext.ACT_LEAKY_RELU, self.f, self.flag.data_ptr()
        for j, h in enumerate(hidden_out or []):
            d.hidden_out[j] = h.data_ptr()
        return op

    def ref(self, X, ctx_rows, sign, dt):
        h = X[:, 32 * self.nk_t:].to(dt) @ self.W[0].to(dt).t() + self.b[0].to(dt)
        h = h + self.b_ctx.to(dt) + ctx_rows.to(dt)[:, None] * self.w_ctx.to(dt)[None, :]
        hs = []
        for j in range(self.nh):
            if j > 0:
                h = h @ self.W[j].to(dt).t() + self.b[j].to(dt)
            h = torch.nn.functional.leaky_relu(h, 0.01)
            hs.append(h)
        return X[:, : 32 * self.nk_t].to(dt) + sign * (h @ self.W[-1].to(dt).t() + self.b[-1].to(dt)), hs


@pytest.mark.parametrize("nk_p,nk_t", [(1, 1), (2, 1), (1, 2)])
@pytest.mark.parametrize("fmt,nh", [("bf16x3", 1), ("bf16x3", 2), ("f16x2", 1), ("f16x2", 2), ("f16x2", 3)])
def test_coupling_planes_ctx_kernel_vs_fp64(fmt, nh, nk_p, nk_t):
    """usf_coupling_planes_ctx through the binding, M in {1, 17, 250} (250 rows: two blocks, the last panel partial) x sign +-1 x
    ctx_stride {0, 1}, LeakyReLU(0.01), against the fp64 formulation on the decoded planes operands; ctx == NULL and
    w_ctx = b_ctx = 0 give the bits of usf_coupling_planes; rows >= M of z stay untouched"""
    ext = _ext()
    L = _Layer(ext, fmt, nh, nk_p, nk_t, seed=100 * nh + 10 * nk_p + nk_t)
    f, nkb = L.f, L.nkb
    K = 256                                                       # the longest contraction of the chain (padded hidden width)
    for M in (1, 17, 250):
        g = torch.Generator().manual_seed(M)
        Mp = -(-M // 16) * 16
        zbuf = torch.zeros(ext.planes_bytes(M, nkb, f), dtype=torch.uint8)
        emulator.planes_encode(_view(zbuf, M, nkb, f), torch.randn(Mp, 32 * nkb, generator=g) * 2, 0)     # (padding rows hold values too)
        Xall = emulator.planes_decode(_view(zbuf, M, nkb, f), Mp)
        X = Xall[:M]
        ctx = (torch.rand(M, generator=g) * 2)
        ctx_d = ctx.to(DEV)

        def run(ctx_args, sign, hidden_out=None, plain=False):
            z = zbuf.to(DEV)
            op = L.op(z, M, sign, hidden_out)
            if plain:
                ext.coupling_planes_op(op, z.device)
            else:
                ext.coupling_planes_ctx_op(op, *ctx_args, z.device)
            torch.cuda.synchronize()
            return z

        for sign in (1.0, -1.0):
            z_plain = run(None, sign, plain=True)
            assert torch.equal(run((None, 0, None, None), sign), z_plain)                                  # ctx == NULL
            z_zero = run((ctx_d, 1, L.dev["zeros"], L.dev["zeros"]), sign)                                   # a zero context layer:
            assert _batch_rows_equal(z_zero, z_plain, M, nkb, f)                                             # the no-context bits in every row of the batch
            assert torch.equal(_pad_rows(z_zero, M, nkb, f), _pad_rows(zbuf, M, nkb, f))
            for stride in (0, 1):
                z = run((ctx_d, stride, L.dev["w_ctx"], L.dev["b_ctx"]), sign)
                got = emulator.planes_decode(_view(z, M, nkb, f), Mp)
                rows = ctx if stride else ctx[:1].expand(M)
                r64, _ = L.ref(X, rows, sign, torch.float64)
                r32, _ = L.ref(X, rows, sign, torch.float32)
                scale = r64.abs().max().item()
                err = (got[:M, : 32 * nk_t].double() - r64).abs().max().item() / scale
                err32 = (r32.double() - r64).abs().max().item() / scale
                print(f"ctx kernel {fmt} nh={nh} nk=({nk_p},{nk_t}) M={M} sign={sign} stride={stride}: err {err:.3e} err32 {err32:.3e}")
                assert err < max(4 * err32, 6e-8 * math.sqrt(K)), (M, sign, stride, err, err32)
                assert err < 1e-5
                assert not torch.equal(z, z_plain)                                                           # the context did enter
                assert torch.equal(got[:M, 32 * nk_t:], X[:, 32 * nk_t:])                                    # conditioning blocks untouched
                assert torch.equal(_pad_rows(z, M, nkb, f), _pad_rows(zbuf, M, nkb, f))                    # rows >= M: the same bytes
                assert torch.equal(got[M:], Xall[M:])
        assert int(L.flag.item()) == 0
    if fmt == "bf16x3":
        # the training forward (hidden_out) with a context: z as the inference launch, hidden_out[l] the layer's activations
        M = 250
        g = torch.Generator().manual_seed(5)
        zbuf = torch.zeros(ext.planes_bytes(M, nkb, f), dtype=torch.uint8)
        emulator.planes_encode(_view(zbuf, M, nkb, f), torch.randn(M, 32 * nkb, generator=g) * 2, 0)
        X = emulator.planes_decode(_view(zbuf, M, nkb, f), M)
        ctx = torch.rand(M, generator=g) * 2
        args = (ctx.to(DEV), 1, L.dev["w_ctx"], L.dev["b_ctx"])
        z0, z1 = zbuf.to(DEV), zbuf.to(DEV)
        hout = [torch.zeros(ext.planes_bytes(M, 8), dtype=torch.uint8, device=DEV) for _ in range(nh)]
        ext.coupling_planes_ctx_op(L.op(z0, M, -1.0), *args, z0.device)
        ext.coupling_planes_ctx_op(L.op(z1, M, -1.0, hout), *args, z1.device)
        torch.cuda.synchronize()
        assert torch.equal(z0, z1)
        _, hs = L.ref(X, ctx, -1.0, torch.float64)
        for l in range(nh):
            got = emulator.planes_decode(_view(hout[l], M, 8, 0), M).double()
            assert ((got - hs[l]).abs().max() / hs[l].abs().max()).item() < 2e-6, l


def test_coupling_planes_ctx_rejects_gate_mode_on_the_device_too():
    ext = _ext()
    L = _Layer(ext, "bf16x3", 1, 1, 1, seed=1)
    z = torch.zeros(ext.planes_bytes(16, 2), dtype=torch.uint8, device=DEV)
    h = torch.zeros(ext.planes_bytes(16, 8), dtype=torch.uint8, device=DEV)
    op = L.op(z, 16, 1.0, [h])
    op.u.coupling_planes.act = ext.ACT_GATE
    op.u.coupling_planes.gate[0] = h.data_ptr()
    with pytest.raises(RuntimeError, match="USF_ACT_GATE"):
        ext.coupling_planes_ctx_op(op, torch.zeros(16, device=DEV), 1, L.dev["w_ctx"], L.dev["b_ctx"], z.device)


# ---- 2. the reference's goldens through the planes plan --------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", ["bf16x3", "f16x2"])
@pytest.mark.parametrize("name", ["synth_d7_k3_soft_ctx", "synth_d7_k3_soft_noctx"])
def test_golden_parity_through_the_planes_plan_with_a_context(name, fmt):
    spec, sd, a = load_case(name)
    flow = build_flow(spec, sd, device=DEV)
    eng = flow.engine()
    _force_planes(eng, fmt)
    eng.use_fused_coupling = True
    ctx = a["context"].to(DEV) if a.get("context") is not None else None
    with torch.no_grad():
        lp = flow.log_prob(a["x"].to(DEV), ctx)                    # (without a context: soft training's noise level 0)
        z = flow.backward(a["x"].to(DEV), ctx) if ctx is not None else flow.backward(a["x"].to(DEV))
        xf = flow._forward(a["zin"].to(DEV), ctx) if ctx is not None else flow._forward(a["zin"].to(DEV))
    plans = _ctx_plans(eng)
    assert plans and all(p["planes_fmt"] == FMT[fmt] for p in plans), "no planes plan with a context was built"
    assert len(plans) == (3 if ctx is not None else 1)
    assert all(_has_ctx_launch(p) for p in plans), "the context coupling launch is not in the planes plan"
    assert any(p.get("n_part", 0) >= 1 for p in plans), "base density was not reduced in the last GEMM's epilogue"
    assert eng.f16_fallbacks == 0
    rel = lambda u, v: ((u.double().cpu() - v.double()).abs() / v.double().abs().clamp_min(1e-30)).max().item()      # noqa: E731
    print(f"golden {name} {fmt}: lp rel64 {rel(lp, a['log_prob64']):.3e} rel32 {rel(lp, a['log_prob32']):.3e}")
    assert rel(lp, a["log_prob64"]) <= 1e-5 and rel(lp, a["log_prob32"]) <= 1e-5, name
    s = max(1.0, a["backward64"].abs().max().item())
    assert (z.cpu().double() - a["backward64"]).abs().max().item() < 2e-5 * s
    s = max(1.0, a["forward64"].abs().max().item())
    assert (xf.cpu().double() - a["forward64"]).abs().max().item() < 2e-5 * s


# ---- 3. ragged row counts --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 17, 8200])
def test_planes_plan_with_a_context_ragged_rows_vs_fp32_plan(B):
    """row counts that are no multiples of the 16-row panels / 128-row blocks: the planes plan with a context == the
    fp32-activation plan with the same context (what served it before), per-row and one-element (broadcast) contexts"""
    spec = orc.FlowSpec(72, 3, [40, 24], soft_training=True)
    sd = orc.synth_state_dict(spec, seed=31)
    flow = build_flow(spec, sd, device=DEV)
    eng = flow.engine()
    fused_default = eng.fused_min_rows
    g = torch.Generator().manual_seed(B)
    x = torch.rand(B, 72, generator=g).to(DEV)
    c = (torch.rand(B, 1, generator=g) * 2).to(DEV)
    c1 = torch.full((1,), 0.7, device=DEV)
    with torch.no_grad():
        _force_planes(eng)
        lp1, z1, lpb1, zb1 = flow.log_prob(x, c), flow.backward(x, c), flow.log_prob(x, c1), flow.backward(x, c1)
        assert len(_ctx_plans(eng)) == 2 and all(_has_ctx_launch(p) for p in _ctx_plans(eng))
        eng.use_planes, eng.fused_min_rows = False, fused_default
        lp2, z2 = flow.log_prob(x, c), flow.backward(x, c)
        lpb2, zb2 = flow.log_prob(x, c1.expand(B, 1).contiguous()), flow.backward(x, c1.expand(B, 1).contiguous())
        assert len(_ctx_plans(eng)) == 2
    for u, v in ((lp1, lp2), (lpb1, lpb2)):
        assert ((u - v).abs() / v.abs()).max().item() < 5e-6
    for u, v in ((z1, z2), (zb1, zb2)):
        assert (u - v).abs().max().item() < 1e-4 * max(1.0, v.abs().max().item())
    assert not torch.equal(lp1, lpb1) or B == 1
    ref = orc.flow_log_prob(orc.to_dtype(sd, torch.float64), spec, x[:64].cpu().double(), c[:64].cpu().double())
    assert ((lp1[:64].cpu().double() - ref).abs() / ref.abs()).max().item() < 1e-5


# ---- 4. sampling -----------------------------------------------------------------------------------------------------------------
def test_sample_with_a_context_draws_from_the_philox_head_and_runs_the_planes_plan():
    ext = _ext()
    spec = orc.FlowSpec(72, 3, [40, 24], soft_training=True)
    flow = build_flow(spec, orc.synth_state_dict(spec, seed=31), device=DEV)
    eng = flow.engine()
    _force_planes(eng)
    n = 300
    c = (torch.rand(n, 1, generator=torch.Generator().manual_seed(2)) * 2).to(DEV)
    before = eng.launch_count
    with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)
        with torch.no_grad():
            x = flow.sample([n], context=c, seed=7)
            z = flow.backward(x, context=c)
            z_other = flow.backward(x, context=c + 0.5)
    assert x.shape == (n, 72) and eng.launch_count > before
    assert any(_has_ctx_launch(p) for p in _ctx_plans(eng))
    info = flow._base_info(torch.device(DEV))
    noise = torch.empty(n, 72, device=DEV)
    ext.base_sample(noise, 72, n, 72, ext.BASE_LAPLACE, info[1], info[2], 7, 0, 0)
    torch.cuda.synchronize()
    scale = max(1.0, noise.abs().max().item())
    assert (z - noise).abs().max().item() < 2e-5 * scale
    assert (z_other - noise).abs().max().item() > 1e-3 * scale
    with torch.no_grad():
        assert torch.equal(flow.sample([n], context=c, seed=7), x) and not torch.equal(flow.sample([n], context=c, seed=8), x)


# ---- 5. the training step --------------------------------------------------------------------------------------------------------
def _train_inputs(B=600, D=160):
    g = torch.Generator().manual_seed(B)
    x = torch.rand(B, D, generator=g)
    ctx = torch.rand(B, 1, generator=g) * 2
    # weights of one sign, as in Flow.fit's loss, different from row to row (tests/test_training_gpu.py)
    g_lp = -(0.5 + torch.rand(B, generator=g)) / B
    return x, ctx, g_lp


def test_planes_training_with_a_context_matches_oracle_autograd():
    """B = 600, D = 160, slope 1 and a Normal base (no kink anywhere): every parameter gradient of the planes training step with
    a context -- layers.1.weight / layers.1.bias of each conditioner included -- within 2e-4 of its tensor's largest entry of
    fp64 autograd through the oracle; a second (replayed) pass gives the same bits"""
    from test_training_gpu import oracle_grads
    spec = orc.FlowSpec(160, 2, [64, 48], soft_training=True, negative_slope=1.0, base="normal")
    sd = orc.synth_state_dict(spec, seed=9)
    flow = build_flow(spec, sd, device=DEV)
    eng = flow.engine()
    _force_planes(eng)
    x, ctx, g_lp = _train_inputs()
    before = eng.launch_count
    lp = flow.log_prob(x.to(DEV), ctx.to(DEV))
    assert lp.requires_grad and eng.launch_count > before
    plan = eng._plan("backward", 600, torch.device(DEV), True, "nat", train=True)
    assert plan.get("planes_train"), "the planes training plan was not chosen"
    assert plan["has_ctx"] and _has_ctx_launch(plan)
    (lp * g_lp.to(DEV)).sum().backward()
    torch.cuda.synchronize()
    lp_ref, g_ref = oracle_grads(spec, sd, x, g_lp, ctx)
    assert ((lp.detach().cpu().double() - lp_ref).abs() / lp_ref.abs()).max().item() <= 1e-5
    checked = []
    for pname, p in flow.named_parameters():
        ref = g_ref.get(pname)
        if not p.requires_grad or ref is None:
            continue
        assert ref.abs().max().item() > 0 and p.grad is not None, pname
        err = (p.grad.cpu().double() - ref.reshape(p.shape)).abs().max().item()
        print(f"ctx train grad {pname}: err/big {err / ref.abs().max().item():.3e}")
        assert err <= 2e-4 * ref.abs().max().item(), (pname, err, ref.abs().max().item())
        checked.append(pname)
    assert sum(".layers.1." in n_ for n_ in checked) == 4 and len(checked) >= 20, checked
    first = {n_: p.grad.clone() for n_, p in flow.named_parameters() if p.grad is not None}
    for p in flow.parameters():
        p.grad = None
    lp2 = flow.log_prob(x.to(DEV), ctx.to(DEV))
    (lp2 * g_lp.to(DEV)).sum().backward()
    torch.cuda.synchronize()
    assert torch.equal(lp2.detach(), lp.detach())
    for n_, p in flow.named_parameters():
        if n_ in first:
            assert torch.equal(p.grad, first[n_]), n_


def test_planes_training_with_a_context_equals_the_fp32_row_path(monkeypatch):
    """the kinked variant (LeakyReLU(0.01), Laplace base): the planes training step with a context against the fp32-row path
    (USFLOWS_AMD_TRAIN_PLANES=0, which served contexts before) -- the same gradients up to summation order / kink flips"""
    spec = orc.FlowSpec(160, 2, [64, 48], soft_training=True)
    sd = orc.synth_state_dict(spec, seed=9)
    x, ctx, _ = _train_inputs()
    res = []
    for on in ("0", "1"):
        monkeypatch.setenv("USFLOWS_AMD_TRAIN_PLANES", on)
        flow = build_flow(spec, sd, device=DEV)
        _force_planes(flow.engine())
        lp = flow.log_prob(x.to(DEV), ctx.to(DEV))
        plan = flow.engine()._plan("backward", 600, torch.device(DEV), True, "nat", train=True)
        assert bool(plan.get("planes_train")) == (on == "1")
        (-lp.mean()).backward()
        torch.cuda.synchronize()
        res.append(({n_: p.grad.clone() for n_, p in flow.named_parameters() if p.grad is not None}, lp.detach()))
    (g0, lp0), (g1, lp1) = res
    assert ((lp0 - lp1).abs() / lp0.abs()).max().item() < 2e-6
    assert g0.keys() == g1.keys() and sum(".layers.1." in n_ for n_ in g0) == 4
    for n_ in g0:
        big = g0[n_].abs().max().item()
        diff = (g0[n_] - g1[n_]).abs()
        n_bad = int((diff > 1e-4 * big + 1e-12).sum().item())
        assert n_bad <= max(2, int(1e-3 * diff.numel())), (n_, n_bad, diff.numel())
        assert diff.max().item() <= 1e-3 * big + 1e-12, (n_, diff.max().item(), big)


# ---- 6. Flow.fit -----------------------------------------------------------------------------------------------------------------
def test_fit_with_soft_training_runs_on_the_planes_training_path(monkeypatch):
    """six SGD steps of Flow.fit(soft_training=True) at batch 600 with the planes training forced: the loss curve of the same fit
    on the fp32-row path, the noise prior's generators seeded alike"""
    import numpy as np
    spec = orc.FlowSpec(160, 2, [64, 48], soft_training=True)
    sd = orc.synth_state_dict(spec, seed=9)
    data = torch.rand(600, 160, generator=torch.Generator().manual_seed(4))
    ds = torch.utils.data.TensorDataset(data, torch.zeros(600))
    curves, planes_used = [], []
    for on in ("0", "1"):
        monkeypatch.setenv("USFLOWS_AMD_TRAIN_PLANES", on)
        flow = build_flow(spec, sd, device=DEV)
        _force_planes(flow.engine())
        torch.manual_seed(12)
        torch.cuda.manual_seed_all(12)
        curves.append(flow.fit(ds, torch.optim.SGD, dict(lr=1e-3), batch_size=600, shuffle=False, device=torch.device(DEV), epochs=6))
        torch.cuda.synchronize()
        planes_used.append(any(p.get("planes_train") and _has_ctx_launch(p) for p in flow.engine()._plans.values()))
    assert planes_used == [False, True]
    print("fit curves", curves)
    assert len(curves[0]) == 6 and np.allclose(curves[1], curves[0], rtol=2e-4, atol=0), curves
