"""Conditional image-shaped flows on the device: usf_conv2d_same_ctx_f32 (the context channel of CondConvNet2D /
CondConvNet's first convolution as a rank-1 epilogue term, reference networks.py:513-680) against fp64 torch, the flows
against the REAL reference's goldens (tests/golden/cond/*.npz), the replayed forms of the layer loop with a context, and
soft-trained unconditional flows on the launches of the same flow without soft training."""
import warnings

import pytest
import torch
import torch.nn.functional as F

from cond_image_cases import cond_case_names, load_cond_case, run_layers
from golden_util import grads_close

DEV = "cuda:0"
pytestmark = pytest.mark.gpu


def _conv_ctx_ref(x, w, b, mask, ctx, act):
    B, C, H, W = x.shape
    a = x.double() * (mask.double().view(1, C, H, W) if mask is not None else 1.0)
    plane = ctx.double().reshape(-1, 1, 1, 1).expand(B, 1, H, W)
    y = F.conv2d(torch.cat([a, plane], 1), w.double(), b.double(), padding=w.shape[-1] // 2)
    return F.leaky_relu(y, act) if act is not None else y


@pytest.mark.parametrize("cin", [3, 4, 16, 48])
def test_conv2d_same_ctx_kernel_vs_fp64(cin):
    from usflows_amd import _ext
    lib = _ext.load()
    g = torch.Generator().manual_seed(cin)
    n = 0
    for cout in (32, 48, 64):
        for ks in (1, 3):
            for H in (6, 7, 8) + ((10,) if cin == 16 and ks == 3 else ()):   # (10 x 10: the unspecialised register-weight kernel)
                if lib.usf_conv2d_same_fits(cin, cout, H, H, ks) < 1:
                    continue
                n += 1
                B = 37 + 13 * ((cout + ks + H) % 5)                         # ragged: not a multiple of any group size
                x = torch.randn(B, cin, H, H, generator=g)
                w = torch.randn(cout, cin + 1, ks, ks, generator=g) / (ks * (cin + 1) ** 0.5)
                bias = 0.1 * torch.randn(cout, generator=g)
                variant = (cout // 16 + ks + H) % 4
                mask = (torch.rand(cin, H, H, generator=g) < 0.5).float() if variant & 1 else None
                act = 0.1 if variant & 2 else None
                for stride in (0, 1):
                    ctx = 2.0 * torch.rand(B if stride else 1, generator=g)
                    xd, wd = x.to(DEV), w.to(DEV)
                    planes = _ext.conv2d_weight_planes(wd[:, :cin].contiguous())
                    y = _ext.conv2d_same_ctx(xd, planes, cout, ks, ctx.to(DEV), wd[:, cin].reshape(cout, -1).contiguous(),
                                             bias=bias.to(DEV), in_mul=None if mask is None else mask.to(DEV).reshape(-1).contiguous(),
                                             out_act=_ext.ACT_LEAKY_RELU if act is not None else _ext.ACT_NONE,
                                             out_slope=act if act is not None else 0.0)
                    ref = _conv_ctx_ref(x, w, bias, mask, ctx.expand(B) if stride == 0 else ctx, act)
                    got = y.cpu().double()
                    s = max(1.0, ref.abs().max().item())
                    border = torch.ones(H, H, dtype=torch.bool)
                    border[1:-1, 1:-1] = False
                    what = (cin, cout, ks, H, B, stride, variant)
                    assert (got - ref)[..., ~border].abs().max().item() <= 1e-5 * s, what
                    assert (got - ref)[..., border].abs().max().item() <= 1e-5 * s, what
    assert n >= 12
    # ctx = NULL: the bits of usf_conv2d_same_f32
    B, cout, H, ks = 41, 32, 7, 3
    x = torch.randn(B, cin, H, H, generator=g).to(DEV)
    w = (torch.randn(cout, cin, ks, ks, generator=g) / (3 * cin ** 0.5)).to(DEV)
    planes = _ext.conv2d_weight_planes(w)
    plain = _ext.conv2d_same(x, planes, cout, ks)
    y = torch.empty_like(plain)
    rc = lib.usf_conv2d_same_ctx_f32(x.data_ptr(), y.data_ptr(), B, cin, cout, H, H, ks, planes.data_ptr(), None, None,
                                     _ext.ACT_NONE, 0.0, _ext.ACT_NONE, 0.0, None, 0, None, _ext.current_stream(x.device))
    torch.cuda.synchronize()
    assert rc == 0 and torch.equal(y, plain)


@pytest.mark.parametrize("ks,H,cout", [(3, 7, 32), (1, 8, 48), (3, 6, 64), (3, 10, 16)])
def test_conv_ctx_wgrad_kernel_vs_fp64_and_deterministic(ks, H, cout):
    from usflows_amd import _ext
    g = torch.Generator().manual_seed(ks * 100 + H)
    for B, stride in ((37, 1), (5, 0), (300, 1)):
        dy = torch.randn(B, cout, H, H, generator=g)
        ctx = 2.0 * torch.rand(B if stride else 1, generator=g)
        # fp64 autograd of the context plane's convolution
        w = torch.zeros(cout, 1, ks, ks, dtype=torch.float64, requires_grad=True)
        plane = ctx.double().reshape(-1, 1, 1, 1).expand(B, 1, H, H)
        (F.conv2d(plane, w, padding=ks // 2) * dy.double()).sum().backward()
        ref = w.grad.reshape(cout, ks * ks)
        dyd, cd = dy.to(DEV), ctx.to(DEV)
        got1 = _ext.conv_ctx_wgrad(dyd, cd, ks)
        got2 = _ext.conv_ctx_wgrad(dyd, cd, ks)
        torch.cuda.synchronize()
        assert torch.equal(got1, got2)                                    # fixed-order sums: the same bits
        assert (got1.cpu().double() - ref).abs().max().item() <= 1e-5 * ref.abs().max().item(), (ks, H, cout, B, stride)


@pytest.mark.parametrize("name", cond_case_names())
def test_cond_image_flow_on_device_matches_reference(name, monkeypatch):
    from usflows_amd import _ext
    calls = []
    real = _ext.conv2d_same_ctx
    monkeypatch.setattr(_ext, "conv2d_same_ctx", lambda *a_, **k_: (calls.append(1), real(*a_, **k_))[1])
    flow, a = load_cond_case(name, device=DEV)
    x, zin, ctx = a["x"].to(DEV), a["zin"].to(DEV), a["ctx"].to(DEV)
    rel = lambda got, want: ((got.cpu().double() - want).abs().max() / want.abs().max()).item()   # noqa: E731
    with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)
        with torch.no_grad():
            assert rel(flow.log_prob(x, ctx), a["log_prob64_ctx"]) <= 1e-5
            assert rel(flow.log_prob(x), a["log_prob64_noctx"]) <= 1e-5
            assert rel(run_layers(flow, x, ctx, True), a["backward64_ctx"]) <= 1e-5
            assert rel(run_layers(flow, zin, ctx, False), a["forward64_ctx"]) <= 1e-5
    n_cpl = sum(1 for l in flow.layers if type(l).__name__ == "MaskedCoupling")
    assert len(calls) >= 4 * n_cpl, "the first convolutions did not run on usf_conv2d_same_ctx_f32"
    if not any(k.startswith("g/") for k in a):
        return
    # gradients of every parameter, the context channel's weight slice included, on the device training path
    wg = []
    real_wg = _ext.conv_ctx_wgrad
    monkeypatch.setattr(_ext, "conv_ctx_wgrad", lambda *a_, **k_: (wg.append(1), real_wg(*a_, **k_))[1])
    flow.zero_grad(set_to_none=True)
    loss = -flow.log_prob(x, ctx).mean()
    loss.backward()
    assert len(wg) == n_cpl, "the context channel's weight gradient did not run on usf_conv_ctx_wgrad_f32"
    assert abs(loss.item() - a["loss64"].item()) <= 1e-5 * abs(a["loss64"].item())
    g_ref = {k[2:]: v for k, v in a.items() if k.startswith("g/")}
    grads_close(dict(flow.named_parameters()), g_ref)


def test_cond_image_flow_replays_with_a_context():
    """64 rows of a CondConvNet2D flow with a per-row context: served by the recorded op list and by the small-batch graph,
    bit-equal to the eager loop; a new context through the same replay gives the eager result of that context"""
    name = "condimage_mnistcfg_c16_7x7_k2_gated_ln_hh1_conj"
    flow, a = load_cond_case(name, device=DEV)
    g = torch.Generator().manual_seed(5)
    x = torch.rand(64, *flow.in_dims, generator=g).to(DEV)
    c1, c2 = (2.0 * torch.rand(64, 1, generator=g)).to(DEV), (2.0 * torch.rand(64, 1, generator=g)).to(DEV)
    with torch.no_grad():
        flow.graph_max_rows, flow.list_max_rows = 0, 0
        e1, e2 = flow.log_prob(x, c1), flow.log_prob(x, c2)
        assert not torch.equal(e1, e2)
        flow.graph_max_rows, flow.list_max_rows = 256, 4096           # the op list
        outs = [flow.log_prob(x, c) for c in (c1, c1, c2, c1)]
        plan = flow._loop_lists[(tuple(x.shape), DEV, "ctx")][1]
        assert plan is not None and plan["ctx_pos"]
        assert torch.equal(outs[0], e1) and torch.equal(outs[1], e1) and torch.equal(outs[2], e2) and torch.equal(outs[3], e1)
        flow.list_max_rows = 0                                        # the small-batch graph
        outs = [flow.log_prob(x, c) for c in (c2, c2, c1)]
        assert (tuple(x.shape), DEV, "ctx") in flow._loop_graphs and not getattr(flow, "_loop_graph_off", False)
        assert torch.equal(outs[0], e2) and torch.equal(outs[1], e2) and torch.equal(outs[2], e1)


def test_soft_trained_convnet2d_flow_takes_the_unconditional_launches(monkeypatch):
    """a soft-trained flow whose conditioners ignore the context (ConvNet2D): bit-equal to the same weights without soft
    training, through the same replayed op list (the context is dropped at the flow)"""
    from golden_util import load_image_case
    flow, a = load_image_case("image_mnistcfg_c16_7x7_k2_gated_ln_hh1_conj", device=DEV)
    x = a["x"].to(DEV).repeat(6, 1, 1, 1)[:64].contiguous()
    with torch.no_grad():
        plain = [flow.log_prob(x) for _ in range(3)]
        flow.soft_training = True
        soft = [flow.log_prob(x) for _ in range(2)] + [flow.log_prob(x, torch.rand(64, 1, device=DEV))]
    assert all(torch.equal(s_, plain[-1]) for s_ in soft)
    assert list(flow._loop_lists) == [(tuple(x.shape), DEV)]          # one list, no context variant


def test_soft_training_fit_of_a_conditional_flow_on_device_matches_torch_autograd(monkeypatch):
    """6 SGD steps at batch 32 of a soft-trained CondConvNet2D flow: the device training path (captured and replayed) against
    torch autograd on the same GPU (image_train off), from the same seed -- the noise and the context come from the same draws"""
    from usflows_amd import _ext
    from usflows_amd.config import config
    name = "condimage_mnistcfg_c16_7x7_k2_gated_ln_hh1_conj"
    data = torch.rand(192, 16, 7, 7, generator=torch.Generator().manual_seed(3))
    ds = torch.utils.data.TensorDataset(data, torch.zeros(data.shape[0]))
    runs = {}
    init = None
    for dev_train in (True, False):
        monkeypatch.setattr(config, "image_train", dev_train)
        flow, _ = load_cond_case(name, device=DEV)
        init = {k: v.detach().cpu().double().clone() for k, v in flow.state_dict().items()}
        wg = []
        real = _ext.conv_ctx_wgrad
        monkeypatch.setattr(_ext, "conv_ctx_wgrad", lambda *a_, **k_: (wg.append(1), real(*a_, **k_))[1])
        torch.manual_seed(0)
        flow.fit(ds, optim=torch.optim.SGD, optim_params=dict(lr=1e-3), batch_size=32, shuffle=False, device=torch.device(DEV),
                 epochs=1)
        monkeypatch.setattr(_ext, "conv_ctx_wgrad", real)
        st = flow.__dict__.get("_train_graph_state") or {}
        runs[dev_train] = ({k: v.detach().cpu().double() for k, v in flow.state_dict().items()}, len(wg), st.get("replays", 0))
    sd_dev, n_wg, replays = runs[True]
    sd_ref, n_wg_ref, _ = runs[False]
    assert n_wg > 0 and n_wg_ref == 0, (n_wg, n_wg_ref)
    assert replays > 0, "the soft-trained step was not captured and replayed"
    # every parameter tensor moved the same way: the two runs differ by under 2 % of what the 6 steps changed (fp32 sums in another
    # order over a 3-block gated conditioner; a missing or wrong gradient column differs by the order of the change itself)
    moved = 0
    for k, v in sd_ref.items():
        change = (v - init[k]).abs().max().item()
        if change == 0.0:
            continue
        moved += 1
        assert (sd_dev[k] - v).abs().max().item() <= 2e-2 * change, (k, (sd_dev[k] - v).abs().max().item(), change)
    assert moved >= 20


def test_sample_with_context_takes_the_radial_head():
    """Flow.sample(shape, context) of a conditional flow with the live configurations' radial base: the Philox radial head,
    then the layers with the context on the device -- the latents come back through the same context with LogNormal radii"""
    import math
    from image_synth import synth_image_params_
    from usflows_amd import distributions as D
    from usflows_amd.flows import USFlow
    from usflows_amd.networks import CondConvNet2D
    dims = [16, 7, 7]
    torch.manual_seed(4)
    nd = D.LogNormal(loc=torch.ones([1]) * 6, scale=torch.ones([1]) * .35, device="cpu")
    base = D.RadialDistribution(device="cpu", p=1.0, loc=torch.zeros(dims), norm_distribution=nd)
    flow = USFlow(base, dims, 2, CondConvNet2D, dict(c_in=16, c_hidden=32, num_layers=1, padding=1, normalize_layers=False,
                                                    gating=False), householder=1, affine_conjugation=True, soft_training=True)
    synth_image_params_(flow, 4)
    flow = flow.to(DEV)
    heads = []
    real = flow._radial_sample_image
    flow._radial_sample_image = lambda *a_, **k_: (heads.append(1), real(*a_, **k_))[1]
    c = (2.0 * torch.rand(64, 1)).to(DEV)
    with torch.no_grad():
        xs = flow.sample([64], context=c, seed=11)
        assert heads and xs.shape == (64, *dims) and torch.isfinite(xs).all()
        z = run_layers(flow, xs, c, True)
        r = z.flatten(1).abs().sum(-1)
        assert (r > math.exp(6 - 1.75)).all() and (r < math.exp(6 + 1.75)).all()
        assert not torch.allclose(run_layers(flow, xs, torch.zeros_like(c), True), z)   # the context matters
        lp = flow.log_prob(xs, c) - flow.base_distribution.log_prob(z)
        assert (lp - lp.mean()).abs().max().item() < 1e-4 * abs(lp.mean().item())
