"""Image-shaped flows (first slice): USFlow(in_dims=[C, H, W]) with the reference's 1x1-conv
BlockAffineTransform, image checkerboard / channel masks and the ConvNet2D conditioner, against outputs of the REAL
reference (tests/golden/image_*.npz).  CPU: the mirror's torch formulation; GPU: the same flows on the device, where every
BlockAffineTransform call runs usf_channel_affine_f32."""
import pytest
import torch

from golden_util import image_case_names, load_image_case
from usflows_amd import transforms as T


def _rel(a, b):
    return ((a.double().cpu() - b.double()).abs() / b.double().abs().clamp_min(1e-30)).max().item()


def _check(flow, a, dev):
    with torch.no_grad():
        lp = flow.log_prob(a["x"].to(dev))
        z = flow.backward(a["x"].to(dev))
        xf = flow._forward(a["zin"].to(dev))
    assert _rel(lp, a["log_prob64"]) < 1e-5 and _rel(lp, a["log_prob32"]) < 1e-5
    s = max(1.0, a["backward64"].abs().max().item())
    assert (z.cpu().double() - a["backward64"]).abs().max().item() < 2e-5 * s
    s = max(1.0, a["forward64"].abs().max().item())
    assert (xf.cpu().double() - a["forward64"]).abs().max().item() < 2e-5 * s
    # uniformly scaling: log_prob(x) - base.log_prob(f^-1(x)) is the parameter-only constant -sum ladj; the 1x1-conv block's
    # log-det counts once per spatial position (transforms.py:980)
    base_lp = torch.distributions.Laplace(0.0, 1.0).log_prob(z.double().cpu()).flatten(1).sum(-1)
    const = lp.double().cpu() - base_lp
    assert (const + float(a["total_ladj64"])).abs().max().item() < 1e-5 * base_lp.abs().max().item()


@pytest.mark.parametrize("name", image_case_names())
def test_image_flow_mirror_matches_reference_cpu(name):
    flow, a = load_image_case(name)
    _check(flow, a, "cpu")
    # masks as the reference builds them (flows.py:494-536)
    m0 = flow.layers[1].mask
    assert m0.shape == (1, *flow.in_dims) and set(m0.unique().tolist()) <= {0.0, 1.0}


@pytest.mark.gpu
@pytest.mark.parametrize("name", image_case_names())
def test_image_flow_on_device_matches_reference(name, monkeypatch):
    from usflows_amd import _ext
    calls, convs = [], []
    real, real_conv = _ext.channel_affine, _ext.conv2d_same
    monkeypatch.setattr(_ext, "channel_affine", lambda *a_, **k_: (calls.append(1), real(*a_, **k_))[1])
    monkeypatch.setattr(_ext, "conv2d_same", lambda x_, pl_, co_, ks_, **k_: (convs.append((x_.shape[1], co_, ks_)),
                                                                             real_conv(x_, pl_, co_, ks_, **k_))[1])
    flow, a = load_image_case(name, device="cuda:0")
    flow.graph_max_rows = 0                      # count the eager loop's launches (the hipGraph path: its own test below)
    flow.merge_image_affine = False              # ... one per affine layer (composed runs: test_image_affine_runs_are_composed)
    _check(flow, a, "cuda:0")
    n_aff = sum(1 for l in flow.layers if type(l).__name__ in ("BlockAffineTransform", "InverseTransform"))
    C = flow.in_dims[0]
    # the 1 x 1-convolution affine layers: usf_channel_affine_f32 up to 16 channels and at the widths with an instance of
    # their own (24 / 32 / 48 / 64: the CIFAR configuration's 48), the matrix-core convolution at other widths
    n_aff_conv = sum(1 for c_ in convs if c_ == (C, C, 1))
    assert len(calls) + n_aff_conv == 3 * n_aff and (n_aff_conv == 0) == (C <= 16 or C in (24, 32, 48, 64)), \
        (len(calls), n_aff_conv, n_aff)
    # the CNN conditioner's convolutions run on usf_conv2d_same_f32
    assert any(c_[2] == 3 for c_ in convs), "the conditioner's 3 x 3 convolutions did not run on the HIP kernel"


@pytest.mark.gpu
@pytest.mark.parametrize("name", image_case_names())
def test_image_affine_runs_are_composed(name, monkeypatch):
    """log_prob of an image-shaped flow composes runs of consecutive 1 x 1-convolution affine layers (block_i^-1 followed by
    block_(i+1) under affine conjugation; the tail block in front of them) into one usf_channel_affine_f32 launch each, behind
    the end-to-end probe: same parity against the reference as the layer-by-layer loop, fewer launches"""
    from usflows_amd import _ext
    flow, a = load_image_case(name, device="cuda:0")
    flow.graph_max_rows = 0
    calls = []
    real = _ext.channel_affine
    monkeypatch.setattr(_ext, "channel_affine", lambda *a_, **k_: (calls.append(1), real(*a_, **k_))[1])
    x = a["x"].to("cuda:0")
    with torch.no_grad():
        flow.merge_image_affine = False
        lp0 = flow.log_prob(x)
        n0 = len(calls)
        flow.merge_image_affine = "auto"
        del calls[:]
        lp1 = flow.log_prob(x)                   # (the probe's two short passes run here)
        del calls[:]
        lp2 = flow.log_prob(x)
        n1 = len(calls)
    log = flow.__dict__.get("merge_guard_log", [])
    n_aff = sum(1 for l in flow.layers if type(l).__name__ in ("BlockAffineTransform", "InverseTransform"))
    conj = any(type(l).__name__ == "InverseTransform" for l in flow.layers)
    if conj and n0 == n_aff:                     # (all affine layers on the channel kernel: C <= 16 or 24 / 32 / 48 / 64)
        assert log and log[-1][0], log           # conditioned parameters: the probe accepts
        assert n1 < n0, (n0, n1)
        # K blocks with conjugation: [tail, A_K fwd], [A_K^-1, A_(K-1) fwd], ... , [A_1^-1]: K + 1 launches instead of 2 K + 1
        assert n1 == (n_aff - 1) // 2 + 1, (n_aff, n1)
    assert torch.equal(lp1, lp2)
    assert _rel(lp1, a["log_prob64"]) < 1e-5 and _rel(lp1, a["log_prob32"]) < 1e-5
    assert (lp1 - lp0).abs().max().item() <= 2e-6 * lp0.abs().max().item()


@pytest.mark.gpu
def test_image_flow_log_prob_does_not_synchronise_the_host():
    """the layer loop (what image-shaped flows run through) enqueues and returns: no pageable host copy, no
    distribution-argument validation on the way (the reference's loop has both: flows.py:236 `torch.zeros(n).to(device)`
    and `base_distribution.log_prob`'s `_validate_sample`) -- at B = 65 536 the two cost 22 of 37 ms per call"""
    name = image_case_names()[0]
    flow, a = load_image_case(name, device="cuda:0")
    x = a["x"].to("cuda:0")
    with torch.no_grad():
        ref = flow.log_prob(x)
        flow.log_prob(x)
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")
        try:
            lp = flow.log_prob(x)
        finally:
            torch.cuda.set_sync_debug_mode("default")
    assert torch.equal(lp, ref)
    # the device base density = the distribution object's (which the CPU run of the same flow uses)
    with torch.no_grad():
        want = flow.base_distribution.log_prob(flow.backward(x))
        got = flow._base_log_prob_layer_loop(flow.backward(x))
    assert got is not None and torch.allclose(got, want, rtol=2e-6, atol=1e-4)


@pytest.mark.gpu
@pytest.mark.parametrize("B,C,P", [(1, 1, 1), (3, 3, 64), (5, 8, 49), (7, 16, 49), (2, 17, 100), (4, 33, 1000), (2, 64, 77),
                                   (65536, 16, 49)])
def test_channel_affine_kernel_vs_conv2d(B, C, P):
    """usf_channel_affine_f32 against F.conv2d with the [C, C, 1, 1] weight (transforms.py:904-962), both directions;
    the last shape is the reference's MNIST configuration (in_dims [16, 7, 7]) at the benchmark batch"""
    from usflows_amd import _ext
    _ext.load()
    g = torch.Generator().manual_seed(B + C + P)
    x = torch.randn(B, C, P, 1, generator=g)
    W = torch.randn(C, C, generator=g) / C ** 0.5
    b = torch.randn(C, generator=g)
    xd = x.to("cuda:0")
    y = torch.full_like(xd, float("nan"))
    _ext.channel_affine(xd, y, W.to("cuda:0"), bias=b.to("cuda:0"))
    idx = torch.unique(torch.cat([torch.arange(min(B, 8)), torch.arange(max(B - 8, 0), B)]))
    ref = torch.nn.functional.conv2d(x[idx].double(), W.double().view(C, C, 1, 1), b.double())
    scale = ref.abs().max().item()
    assert not torch.isnan(y).any()
    assert (y[idx.to("cuda:0")].cpu().double() - ref).abs().max().item() < 2e-6 * scale
    _ext.channel_affine(xd, y, W.to("cuda:0"), pre_sub=b.to("cuda:0"))
    ref = torch.nn.functional.conv2d(x[idx].double() - b.double().view(1, C, 1, 1), W.double().view(C, C, 1, 1))
    assert (y[idx.to("cuda:0")].cpu().double() - ref).abs().max().item() < 2e-6 * max(scale, ref.abs().max().item())
    with pytest.raises(RuntimeError):
        _ext.channel_affine(xd, xd, W.to("cuda:0"))           # in place is rejected


@pytest.mark.gpu
@pytest.mark.parametrize("B,C,P", [(1, 1, 1), (3, 5, 49), (7, 32, 49), (2, 64, 100), (4097, 16, 49)])
def test_image_elementwise_kernels_vs_torch(B, C, P):
    """usf_layernorm_channels_f32 (with and without the folded (Leaky)ReLU), usf_gated_residual_f32 and
    usf_masked_residual_f32 against the torch formulas of the reference's modules (networks.py:40-58, 108-122;
    transforms.py:277-306) in fp64"""
    from usflows_amd import _ext
    _ext.load()
    g = torch.Generator().manual_seed(B * 7 + C + P)
    x = torch.randn(B, C, P, 1, generator=g) * 3
    gamma, beta = torch.randn(C, generator=g), torch.randn(C, generator=g)
    xd = x.to("cuda:0")
    for act, slope, f in ((_ext.ACT_NONE, 0.0, lambda v: v), (_ext.ACT_LEAKY_RELU, 0.0, torch.relu),
                          (_ext.ACT_LEAKY_RELU, 0.01, lambda v: torch.nn.functional.leaky_relu(v, 0.01))):
        a = f(x.double())
        mean, var = a.mean(dim=1, keepdim=True), a.var(dim=1, unbiased=False, keepdim=True)
        ref = (a - mean) / torch.sqrt(var + 1e-5) * gamma.double().view(1, C, 1, 1) + beta.double().view(1, C, 1, 1)
        got = _ext.layernorm_channels(xd, gamma.to("cuda:0"), beta.to("cuda:0"), 1e-5, act, slope)
        assert (got.cpu().double() - ref).abs().max().item() < 1e-5 * max(1.0, ref.abs().max().item())
    vg = torch.randn(B, 2 * C, P, 1, generator=g) * 2
    ref = x.double() + vg[:, :C].double() * torch.sigmoid(vg[:, C:].double())
    got = _ext.gated_residual(xd, vg.to("cuda:0"))
    assert (got.cpu().double() - ref).abs().max().item() < 2e-6 * max(1.0, ref.abs().max().item())
    t = torch.randn(B, C, P, 1, generator=g)
    om = (torch.rand(C * P, generator=g) > 0.5).float()
    for sign in (1.0, -1.0):
        ref = x.double() + sign * om.double().view(1, C, P, 1) * t.double()
        got = _ext.masked_residual(xd, t.to("cuda:0"), om.to("cuda:0"), sign)
        assert torch.equal(got.cpu().double(), ref.float().double())


@pytest.mark.gpu
@pytest.mark.parametrize("B,cin,cout,H,W,ks", [(1, 1, 1, 1, 1, 1), (3, 16, 32, 7, 7, 3), (5, 32, 32, 7, 7, 3), (4, 32, 64, 7, 7, 1),
                                               (9, 32, 16, 7, 7, 3), (2, 48, 32, 8, 8, 3), (3, 4, 32, 14, 14, 3), (2, 5, 7, 3, 9, 3),
                                               (2, 32, 32, 16, 16, 3), (2, 64, 64, 5, 5, 1), (7, 33, 17, 5, 6, 1), (4099, 16, 32, 7, 7, 3)])
def test_conv2d_same_kernel_vs_torch(B, cin, cout, H, W, ks):
    """usf_conv2d_same_f32 (implicit GEMM on the bf16 matrix cores, bf16x3 arithmetic) against F.conv2d in fp64: the
    conditioner shapes of the reference's MNIST / CIFAR configurations (networks.py:405-510), ragged sizes, the folded
    input (Leaky)ReLU, the folded coupling mask and the output activation"""
    import torch.nn.functional as F
    from usflows_amd import _ext
    _ext.load()
    lib = _ext.load()
    assert lib.usf_conv2d_same_fits(cin, cout, H, W, ks) > 0 and lib.usf_conv2d_same_fits(64, 64, 16, 16, 3) == 0
    g = torch.Generator().manual_seed(B + cin * 3 + cout * 5 + H + ks)
    x = torch.randn(B, cin, H, W, generator=g) * 2
    w = torch.randn(cout, cin, ks, ks, generator=g) / (cin * ks * ks) ** 0.5
    b = torch.randn(cout, generator=g)
    mask = (torch.rand(cin, H, W, generator=g) > 0.5).float()
    planes = _ext.conv2d_weight_planes(w.to("cuda:0"))
    xd = x.to("cuda:0")
    rows = torch.unique(torch.cat([torch.arange(min(B, 6)), torch.arange(max(B - 6, 0), B)]))
    for in_act, in_slope, use_mask, out_act in ((_ext.ACT_NONE, 0.0, False, _ext.ACT_NONE), (_ext.ACT_LEAKY_RELU, 0.0, False, _ext.ACT_NONE),
                                                (_ext.ACT_NONE, 0.0, True, _ext.ACT_LEAKY_RELU), (_ext.ACT_LEAKY_RELU, 0.01, True, _ext.ACT_NONE)):
        a = x[rows].double()
        if in_act == _ext.ACT_LEAKY_RELU:
            a = F.leaky_relu(a, in_slope)
        if use_mask:
            a = a * mask.double()
        ref = F.conv2d(a, w.double(), b.double(), padding=ks // 2)
        if out_act == _ext.ACT_LEAKY_RELU:
            ref = F.leaky_relu(ref, 0.0)
        got = _ext.conv2d_same(xd, planes, cout, ks, bias=b.to("cuda:0"), in_mul=mask.reshape(-1).to("cuda:0") if use_mask else None,
                               in_act=in_act, in_slope=in_slope, out_act=out_act, out_slope=0.0)
        assert got.shape == (B, cout, H, W) and not torch.isnan(got).any()
        err = (got[rows.to("cuda:0")].cpu().double() - ref).abs().max().item()
        assert err < 3e-6 * max(1.0, ref.abs().max().item()), (in_act, use_mask, out_act, err)
    # no bias
    got = _ext.conv2d_same(xd, planes, cout, ks)
    ref = F.conv2d(x[rows].double(), w.double(), None, padding=ks // 2)
    assert (got[rows.to("cuda:0")].cpu().double() - ref).abs().max().item() < 3e-6 * max(1.0, ref.abs().max().item())


@pytest.mark.gpu
def test_conv2d_same_kernel_random_shapes():
    """40 random shapes the kernel accepts (channels 1..64, H * W <= 256, kernel 1 or 3, batches that leave the last
    sample group ragged) against F.conv2d in fp64"""
    import random
    import torch.nn.functional as F
    from usflows_amd import _ext
    lib = _ext.load()
    rnd = random.Random(1234)
    g = torch.Generator().manual_seed(99)
    done = 0
    while done < 40:
        cin, cout, ks = rnd.randint(1, 64), rnd.randint(1, 64), rnd.choice([1, 3])
        H = rnd.randint(1, 16)
        W = rnd.randint(1, min(16, 256 // H))
        B = rnd.randint(1, 40)
        if lib.usf_conv2d_same_fits(cin, cout, H, W, ks) < 1:
            continue
        x = torch.randn(B, cin, H, W, generator=g)
        w = torch.randn(cout, cin, ks, ks, generator=g) / (cin * ks * ks) ** 0.5
        b = torch.randn(cout, generator=g)
        got = _ext.conv2d_same(x.to("cuda:0"), _ext.conv2d_weight_planes(w.to("cuda:0")), cout, ks, bias=b.to("cuda:0"),
                               in_act=_ext.ACT_LEAKY_RELU, in_slope=0.1)
        ref = F.conv2d(F.leaky_relu(x.double(), 0.1), w.double(), b.double(), padding=ks // 2)
        err = (got.cpu().double() - ref).abs().max().item()
        assert err < 3e-6 * max(1.0, ref.abs().max().item()), (B, cin, cout, H, W, ks, err)
        done += 1


@pytest.mark.gpu
@pytest.mark.parametrize("B,C,ch,H,W", [(5, 32, 32, 7, 7), (3, 8, 8, 6, 6), (4, 6, 6, 8, 8), (1000, 32, 32, 7, 7), (2, 20, 12, 5, 5)])
def test_gated_conv_module_on_device_vs_torch(B, C, ch, H, W):
    """GatedConv (networks.py:61-122) on the device -- first convolution with the ReLU folded in, second convolution fused
    with the gate (value / gate rows packed pairwise; channel counts that fill, half-fill and straddle the 16-row tiles)
    -- against the same module's torch formulation in fp64"""
    import copy
    from usflows_amd.networks import GatedConv
    torch.manual_seed(B + C + H)
    m = GatedConv(C, ch, kernel_size=3, padding="same")
    x = torch.randn(B, C, H, W) * 2
    ref = copy.deepcopy(m).double()(x.double())
    md = m.to("cuda:0")
    with torch.no_grad():
        got = md(x.to("cuda:0"))
    assert (got.cpu().double() - ref).abs().max().item() < 5e-6 * max(1.0, ref.abs().max().item())


@pytest.mark.gpu
@pytest.mark.parametrize("name", image_case_names())
def test_small_batch_layer_loop_replays_a_hip_graph(name):
    """log_prob of <= 256 rows of an image-shaped flow: captured once per (shape, parameter versions) -- at its second sighting --, replayed afterwards --
    bit-equal to the eager loop, recaptured after an in-place parameter update, a second shape gets a graph of its own"""
    flow, a = load_image_case(name, device="cuda:0")
    flow.list_max_rows = 0                       # (the op-list form would serve these calls first: its own test below)
    x = a["x"].to("cuda:0")
    with torch.no_grad():
        flow.graph_max_rows = 0
        eager = flow.log_prob(x)
        eager_half = flow.log_prob(x[: x.shape[0] // 2])
        flow.graph_max_rows = 256
        g1 = flow.log_prob(x)
        g2 = flow.log_prob(x)
        assert len(flow._loop_graphs) == 1 and not getattr(flow, "_loop_graph_off", False)
        assert torch.equal(g1, eager) and torch.equal(g2, eager)
        # (a (shape, parameter version) pair is captured the second time it is seen: the first call runs the eager loop)
        assert torch.equal(flow.log_prob(x[: x.shape[0] // 2]), eager_half) and len(flow._loop_graphs) == 1
        assert torch.equal(flow.log_prob(x[: x.shape[0] // 2]), eager_half) and len(flow._loop_graphs) == 2
        for p in flow.parameters():
            if p.numel() > 1:
                p.mul_(1.0 + 1e-3)
        flow.graph_max_rows = 0
        eager2 = flow.log_prob(x)
        flow.graph_max_rows = 256
        assert torch.equal(flow.log_prob(x), eager2) and not torch.equal(eager2, eager)
        assert torch.equal(flow.log_prob(x), eager2)            # second sighting of the new versions: recaptured, replayed
    # under autograd the eager (composite) loop serves the call
    lp = flow.log_prob(x)
    assert lp.requires_grad


@pytest.mark.gpu
@pytest.mark.parametrize("name", image_case_names())
def test_layer_loop_runs_as_one_op_list(name, monkeypatch):
    """log_prob of an image-shaped batch as ONE usf_run_ops call (USF_OP_CALL entries recorded from the eager loop at the second
    sighting of a (shape, parameter version) pair): bit-equal to the eager loop, on fresh inputs too, re-recorded after an
    in-place parameter update; flows with a layer the kernels do not serve (a torch op inside the pass) are recognised and
    keep the eager loop / the hipGraph"""
    from usflows_amd import _ext
    flow, a = load_image_case(name, device="cuda:0")
    x = a["x"].to("cuda:0")
    x2 = (x * 0.5 + 0.25).contiguous()
    runs = []
    real = _ext.run_ops
    monkeypatch.setattr(_ext, "run_ops", lambda ops, n, dev=None: (runs.append(n), real(ops, n, dev))[1])
    with torch.no_grad():
        flow.graph_max_rows = 0
        eager, eager2 = flow.log_prob(x), flow.log_prob(x2)
        flow.graph_max_rows = 256
        assert torch.equal(flow.log_prob(x), eager)   # first sighting of (shape, versions) with the replay forms on: eager loop
        r1 = flow.log_prob(x)                    # second sighting: recorded while it runs
        plan = flow._loop_lists[(tuple(x.shape), "cuda:0")][1]
        served = plan is not None                # (a pass with a torch op inside -- a shape a kernel does not serve -- keeps the loop)
        assert served or not any(k in name for k in ("mnistcfg", "cifarcfg", "c16_7x7")), name
        r2, r3 = flow.log_prob(x), flow.log_prob(x2)
        assert torch.equal(r1, eager) and torch.equal(r2, eager) and torch.equal(r3, eager2)
        if served:
            assert runs == [plan["n"], plan["n"]] and plan["n"] >= 10, runs
            # an in-place parameter update: new versions -> eager call, then a new recording
            for p in flow.parameters():
                if p.numel() > 1:
                    p.mul_(1.0 + 1e-3)
            flow.graph_max_rows = 0
            e3 = flow.log_prob(x)
            flow.graph_max_rows = 256
            for _ in range(4):                    # eager (first sighting), recorded, replayed, replayed
                assert torch.equal(flow.log_prob(x), e3)
            assert len(runs) == 4 and not torch.equal(e3, eager)
        else:
            assert runs == []
    _check(flow, a, "cuda:0") if not served else None


def _fit_twice(make_flow, data, optim, optim_params, batch_size, epochs):
    """Flow.fit from the same start with the graphed training step and with eager steps"""
    import copy
    import numpy as np
    f_graph = make_flow().to("cuda:0")
    f_eager = copy.deepcopy(f_graph)
    f_eager.use_train_graph = False
    ds = torch.utils.data.TensorDataset(data, torch.zeros(data.shape[0]))
    out = []
    for f in (f_graph, f_eager):
        np.random.seed(5)
        out.append(f.fit(ds, optim=optim, optim_params=optim_params, batch_size=batch_size, shuffle=True,
                         device=torch.device("cuda:0"), epochs=epochs))
    return f_graph, f_eager, out[0], out[1]


@pytest.mark.gpu
@pytest.mark.parametrize("optim", ["sgd", "sophia"])
def test_fit_replays_the_training_step_of_an_image_flow_as_a_hip_graph(optim):
    """Flow.fit on an image-shaped flow (composite torch formulation under autograd): after three eager steps the whole
    step -- gradient zeroing, log_prob, backward, optimiser update -- is one hipGraph replay; the ragged last batch of each
    epoch runs eagerly; same losses and parameters as eager steps from the same start (SGD: to rounding; SophiaG: its
    update is lr * sign(m) while the Hessian estimate is zero, so single elements may differ by 2 lr)"""
    from usflows_amd.flows import USFlow
    from usflows_amd.networks import ConvNet2D
    from usflows_amd.sophia import SophiaG
    dims = [4, 6, 6]

    def make_flow():
        torch.manual_seed(3)
        base = torch.distributions.Laplace(torch.zeros(dims, device="cuda:0"), torch.ones(dims, device="cuda:0"))
        return USFlow(base, dims, 2, ConvNet2D, dict(c_in=4, c_hidden=8, num_layers=1, padding="same", kernel_size=3,
                                                    normalize_layers=True, gating=True, nonlinearity=torch.nn.ReLU()),
                      householder=1, affine_conjugation=True)

    def tamed():
        # (the reference's default initialisation is ill-conditioned -- SURVEY 7-H2: losses of 1e5 that amplify the last-bit
        # run-to-run differences of the convolution's atomically accumulated weight gradients; compare on a tame start)
        f = make_flow()
        g = torch.Generator().manual_seed(4)
        with torch.no_grad():
            for m in f.modules():
                if isinstance(m, T.LUTransform):
                    d = m.dim
                    m.L_raw.copy_(torch.eye(d) + 0.1 * torch.randn(d, d, generator=g).tril(-1))
                    m.U_raw.copy_(torch.diag(0.75 + 0.5 * torch.rand(d, generator=g)) + 0.1 * torch.randn(d, d, generator=g).triu(1))
                elif isinstance(m, T.ScaleTransform):
                    m.scale.fill_(1.0)
        return f

    data = torch.rand(8 * 16 + 5, *dims, generator=torch.Generator().manual_seed(1))
    cls, params = (torch.optim.SGD, dict(lr=1e-4)) if optim == "sgd" else (SophiaG, dict(lr=1e-5))
    fg, fe, lg, le = _fit_twice(tamed, data, cls, params, 16, 2)
    st = fg._train_graph_state
    assert st["graph"] is not None and st["replays"] == (8 - 3) + 8, st["replays"]
    assert "_train_graph_state" not in fe.__dict__
    # the eager steps behind the capture (the ragged last batch of each epoch) left the graph's gradient buffers in place:
    # `zero_grad()` there would free what the replays write to
    assert all(g is None or p.grad is g for p, g in zip(st["params"], st["keep"][0]))
    if optim == "sophia":
        assert all(v[1].data_ptr() == st["keep"][1][k][1].data_ptr() for k, v in st["optim"]._tables.items())
    assert lg[1] < lg[0]
    for a, b in zip(lg, le):
        assert abs(a - b) <= 2e-5 * abs(b), (lg, le)
    tol = 2e-5 if optim == "sgd" else 2.5e-5
    for (k, a), (_, b) in zip(fg.state_dict().items(), fe.state_dict().items()):
        assert (a - b).abs().max().item() <= tol * max(1.0, b.abs().max().item()), k
    # the version-keyed caches of the inference path see the replayed updates: device log_prob == the torch composite
    x = data[:7].to("cuda:0")
    with torch.no_grad():
        lp = fg.log_prob(x)
        fg.graph_max_rows = 0
        ref = fg._layer_loop_log_prob(x)
    assert ((lp - ref).abs() / ref.abs()).max().item() < 1e-5


@pytest.mark.gpu
def test_fit_graph_serves_flat_flows_without_a_device_backward():
    """a flat flow whose conditioner has no HIP backward (the gated / layer-normalised vector ConvNet): Flow.fit's steps are
    the torch composite under autograd -- replayed as a graph like the image-shaped flows', same result as eager steps"""
    from oracle import usflows_oracle as orc
    from model_util import build_flow
    spec = orc.FlowSpec(12, 2, [16, 16], householder=1, conditioner="ConvNet", extra={"gating": True, "normalize_layers": True})
    sd = orc.synth_state_dict(spec, seed=9)
    data = torch.rand(6 * 8, 12, generator=torch.Generator().manual_seed(2))
    fg, fe, lg, le = _fit_twice(lambda: build_flow(spec, sd, device="cuda:0"), data, torch.optim.SGD, dict(lr=1e-3), 8, 1)
    assert fg._train_graph_state["replays"] == 3
    for a, b in zip(lg, le):
        assert abs(a - b) <= 1e-5 * abs(b), (lg, le)
    for (k, a), (_, b) in zip(fg.state_dict().items(), fe.state_dict().items()):
        assert (a - b).abs().max().item() <= 1e-6 * max(1.0, b.abs().max().item()), k


@pytest.mark.gpu
@pytest.mark.parametrize("B", [0, 1, 3, 65, 257, 1000])
def test_image_flow_empty_and_ragged_batches_on_device(B):
    """empty, single-row and ragged batches of an image-shaped flow (groups of samples that do not fill the convolution
    kernel's LDS image, partial waves of the per-pixel kernels; 257 rows: one past the hipGraph path's limit): the device
    path against the torch formulation of the same modules on the CPU, round trip"""
    name = [n for n in image_case_names() if "mnistcfg" in n][0]
    flow_cpu, _ = load_image_case(name)
    flow, _ = load_image_case(name, device="cuda:0")
    x = torch.rand(B, *flow.in_dims, generator=torch.Generator().manual_seed(B + 1))
    with torch.no_grad():
        z = flow.backward(x.to("cuda:0"))
        xr = flow._forward(z)
        assert z.shape == x.shape and xr.shape == x.shape
        if B == 0:
            # torch's Independent cannot sum an empty image batch (`reshape(0, -1)`): the reference raises here, and so do the
            # mirror on the CPU and the device path (same error behaviour); the transforms themselves pass empty batches
            with pytest.raises(RuntimeError):
                flow_cpu.log_prob(x)
            with pytest.raises(RuntimeError):
                flow.log_prob(x.to("cuda:0"))
            return
        lp = flow.log_prob(x.to("cuda:0"))
        ref = flow_cpu.log_prob(x)
    assert lp.shape == (B,)
    assert _rel(lp.cpu(), ref) < 1e-5
    assert (xr.cpu() - x).abs().max().item() < 1e-4


@pytest.mark.gpu
@pytest.mark.parametrize("gated", [True, False])
@pytest.mark.parametrize("B,cin,cout,H,W", [(1, 8, 2, 1, 1), (5, 32, 64, 7, 7), (3, 16, 32, 7, 7), (1000, 32, 64, 7, 7), (7, 48, 96, 8, 8),
                                            (2, 24, 10, 5, 3), (4, 64, 256, 4, 4), (130, 32, 32, 14, 14)])
def test_pointwise_conv_kernel_vs_torch(B, cin, cout, H, W, gated):
    """usf_pointwise_conv_f32 (1 x 1 convolution on the vector ALUs, exact fp32) against F.conv2d in fp64: plain with
    bias / activations, and GatedConv's `x + val * sigmoid(gate)` form (networks.py:108-122)"""
    from usflows_amd import _ext
    g = torch.Generator().manual_seed(B * 1000 + cin + cout)
    dev = "cuda:0"
    x = torch.randn(B, cin, H, W, generator=g).to(dev)
    w = (torch.randn(cout, cin, generator=g) / cin ** 0.5).to(dev)
    b = torch.randn(cout, generator=g).to(dev)
    a = torch.nn.functional.leaky_relu(x.double(), 0.01)
    full = torch.nn.functional.conv2d(a, w.double().view(cout, cin, 1, 1), b.double())
    if gated:
        C = cout // 2
        gx = torch.randn(B, C, H, W, generator=g).to(dev)
        ref = gx.double() + full[:, :C] * torch.sigmoid(full[:, C:])
        y = _ext.pointwise_conv(x, w, b, in_act=_ext.ACT_LEAKY_RELU, in_slope=0.01, gate_x=gx)
    else:
        ref = torch.relu(full)
        y = _ext.pointwise_conv(x, w, b, in_act=_ext.ACT_LEAKY_RELU, in_slope=0.01, out_act=_ext.ACT_LEAKY_RELU, out_slope=0.0)
    torch.cuda.synchronize()
    assert y.shape == ref.shape
    assert (y.double() - ref).abs().max().item() < 3e-6 * max(1.0, ref.abs().max().item())
    # without bias / activations
    y2 = _ext.pointwise_conv(x, w) if not gated else None
    if y2 is not None:
        ref2 = torch.nn.functional.conv2d(x.double(), w.double().view(cout, cin, 1, 1))
        assert (y2.double() - ref2).abs().max().item() < 3e-6 * max(1.0, ref2.abs().max().item())


@pytest.mark.gpu
def test_pointwise_conv_rejects_what_it_does_not_serve():
    from usflows_amd import _ext
    x = torch.zeros(2, 20, 3, 3, device="cuda:0")
    assert not _ext.pointwise_conv_supported(20, 8) and _ext.pointwise_conv_supported(32, 64, True)
    assert not _ext.pointwise_conv_supported(32, 63, True) and not _ext.pointwise_conv_supported(32, 300)
    with pytest.raises(RuntimeError):
        _ext.pointwise_conv(x, torch.zeros(8, 20, device="cuda:0"))


@pytest.mark.gpu
@pytest.mark.parametrize("B,C,H,W", [(1, 8, 1, 1), (5, 32, 7, 7), (3, 16, 7, 7), (1000, 32, 7, 7), (7, 24, 8, 8), (130, 32, 14, 14)])
def test_pointwise_conv_gated_layernorm_form_vs_torch(B, C, H, W):
    """usf_pointwise_conv_f32 with the layer norm joined to the gated pass: GatedConv's `x + val * sigmoid(gate)`, the ReLU
    and the LayerNormChannels behind it (networks.py:108-122, 480-493, 40-58) against the torch fp64 formulation, and
    bit-equal to the two-pass device form (gated pointwise pass, then usf_layernorm_channels_f32 with the ReLU folded in)
    where that pass is the one-thread-per-pixel kernel (more than 16 384 pixels)"""
    from usflows_amd import _ext
    g = torch.Generator().manual_seed(B * 100 + C)
    dev = "cuda:0"
    x = torch.randn(B, C, H, W, generator=g).to(dev)
    gx = torch.randn(B, C, H, W, generator=g).to(dev)
    w = (torch.randn(2 * C, C, generator=g) / C ** 0.5).to(dev)
    b = torch.randn(2 * C, generator=g).to(dev)
    gamma, beta = (0.5 + torch.rand(C, generator=g)).to(dev), torch.randn(C, generator=g).to(dev)
    a = torch.relu(x.double())
    full = torch.nn.functional.conv2d(a, w.double().view(2 * C, C, 1, 1), b.double())
    r = torch.relu(gx.double() + full[:, :C] * torch.sigmoid(full[:, C:]))
    mean = r.mean(dim=1, keepdim=True)
    var = r.var(dim=1, unbiased=False, keepdim=True)
    ref = (r - mean) / torch.sqrt(var + 1e-5) * gamma.double().view(1, C, 1, 1) + beta.double().view(1, C, 1, 1)
    relu = (_ext.ACT_LEAKY_RELU, 0.0)
    y = _ext.pointwise_conv(x, w, b, in_act=relu[0], in_slope=relu[1], out_act=relu[0], out_slope=relu[1], gate_x=gx,
                            ln=(gamma, beta, 1e-5))
    two = _ext.layernorm_channels(_ext.pointwise_conv(x, w, b, in_act=relu[0], in_slope=relu[1], gate_x=gx), gamma, beta, 1e-5,
                                  relu[0], relu[1])
    torch.cuda.synchronize()
    assert (y.double() - ref).abs().max().item() < 2e-5 * max(1.0, ref.abs().max().item())
    if B * H * W > 16384 or C <= 8:
        assert torch.equal(y, two)
    else:
        # few pixels: the stand-alone layer norm runs eight lanes per pixel (another order of additions): equal to rounding
        assert (y - two).abs().max().item() < 4e-6 * max(1.0, ref.abs().max().item())
        assert (two.double() - ref).abs().max().item() < 2e-5 * max(1.0, ref.abs().max().item())
    with pytest.raises(RuntimeError):
        _ext.pointwise_conv(x, w, b, ln=(gamma, beta, 1e-5))             # the layer-norm form needs the gated mode


@pytest.mark.gpu
def test_convnet2d_joins_gated_conv_relu_and_layernorm_into_one_pass(monkeypatch):
    """ConvNet2D on the device: [GatedConv, ReLU, LayerNormChannels] runs as conv 3x3 + ONE pointwise pass (no separate layer
    norm launch); same values as with config.pointwise = False (matrix-core 1 x 1 convolution + layer-norm pass) to rounding and as the
    torch modules on the CPU"""
    from usflows_amd import _ext
    from usflows_amd.networks import ConvNet2D
    torch.manual_seed(2)
    net = ConvNet2D(16, c_hidden=32, num_layers=2, padding="same", kernel_size=3, normalize_layers=True, gating=True,
                    nonlinearity=torch.nn.ReLU())
    x = torch.randn(37, 16, 7, 7)
    with torch.no_grad():
        ref = net(x)
        dnet = net.to("cuda:0")
        ln_calls = []
        real = _ext.layernorm_channels
        monkeypatch.setattr(_ext, "layernorm_channels", lambda *a_, **k_: (ln_calls.append(1), real(*a_, **k_))[1])
        y = dnet(x.to("cuda:0"))
        assert not ln_calls, "the layer norm ran as a pass of its own"
        from usflows_amd.config import config
        monkeypatch.setattr(config, "pointwise", False)
        y0 = dnet(x.to("cuda:0"))
        assert len(ln_calls) == 2
    assert (y.cpu() - ref).abs().max().item() < 2e-5 * max(1.0, ref.abs().max().item())
    assert (y - y0).abs().max().item() < 2e-5 * max(1.0, ref.abs().max().item())


@pytest.mark.gpu
def test_layer_loop_log_det_total_is_cached_per_parameter_version(monkeypatch):
    """the layer loop's sum of parameter-only log-determinants (Flow._parameter_only_ladj_total): same log_prob as the loop
    that asks every layer on every call, recomputed after an in-place parameter update, not used under autograd nor for a
    flow with the affine-coupling extension (whose log-det depends on the sample)"""
    from usflows_amd.flows import Flow
    name = [n for n in image_case_names() if "mnistcfg" in n][0]
    flow, a = load_image_case(name, device="cuda:0")
    flow.graph_max_rows = 0
    x = a["x"].to("cuda:0")

    def both():
        with torch.no_grad():
            cached = flow.log_prob(x)
            assert flow.__dict__.get("_ladj_total_cache") is not None
            with monkeypatch.context() as m:
                m.setattr(Flow, "_parameter_only_ladj_total", lambda self, x_: None)
                plain = flow.log_prob(x)
        return cached, plain

    c1, p1 = both()
    assert _rel(c1, p1.cpu()) < 1e-6 and _rel(c1, a["log_prob64"]) < 1e-5
    key1 = flow._ladj_total_cache[0]
    with torch.no_grad():
        flow.layers[-1].scale.mul_(1.25)
    c2, p2 = both()
    assert flow._ladj_total_cache[0] != key1 and _rel(c2, p2.cpu()) < 1e-6 and (c2 - c1).abs().min().item() > 1.0
    with torch.no_grad():
        assert flow._parameter_only_ladj_total(x) is not None
    with torch.enable_grad():
        assert flow._parameter_only_ladj_total(x) is None              # parameters require grad: nothing is cached


@pytest.mark.gpu
def test_log_det_cache_is_not_used_with_the_affine_coupling_extension():
    from usflows_amd.flows import _ladj_is_parameter_only
    from usflows_amd import transforms as T_
    assert _ladj_is_parameter_only(T_.ScaleTransform([4])) and _ladj_is_parameter_only(T_.BlockAffineTransform([4], T_.LUTransform(4)))
    assert _ladj_is_parameter_only(T_.InverseTransform(T_.BlockAffineTransform([4], T_.LUTransform(4))))
    amc = T_.AffineMaskedCoupling(torch.tensor([[1.0, 0.0, 1.0, 0.0]]), torch.nn.Linear(4, 8))
    assert not _ladj_is_parameter_only(amc) and not _ladj_is_parameter_only(T_.InverseTransform(amc))


# ---------------------------------------------------------------------------------------------------------------------
# Full-size parity (round-2 review, "what's weak" 1): the image path at the batch its performance is quoted at.
# ---------------------------------------------------------------------------------------------------------------------
FULL_ROWS = 65536


@pytest.mark.gpu
@pytest.mark.parametrize("name,rows", [("image_mnistcfg_c16_7x7_k2_gated_ln_hh1_conj_synth", FULL_ROWS),
                                       ("image_mnistcfg_c16_7x7_k2_gated_ln_hh1_conj", FULL_ROWS),
                                       ("image_cifarcfg_full_c48_8x8_k10_gated_ln_hh0_conj_synth", 16384)])
def test_image_flow_full_batch_head_middle_tail_vs_reference(name, rows):
    """The reference's golden rows placed at the head, the middle and the tail of a full batch (65 536 rows of the MNIST
    configuration, tests/explib/mnist.yaml:44-77; 16 384 of the whole 10-block CIFAR configuration,
    experiments/cifar/cifar.yaml:56-77): the persistent convolution kernel walks > 1 000 sample groups per block there,
    a regime the small cases never reach.  log_prob / backward at those rows against the reference's fp64 and fp32
    runs; on the WHOLE batch: the UDL constant (log_prob(x) - base.log_prob(f^-1(x)) == -sum ladj, one number for all
    rows) and the round trip _forward(backward(x)) == x."""
    flow, a = load_image_case(name, device="cuda:0")
    n = a["x"].shape[0]
    g = torch.Generator().manual_seed(4321)
    x = torch.rand(rows, *flow.in_dims, generator=g)
    third = n // 3
    spots = [(0, 0, third), (rows // 2 - 7, third, 2 * third), (rows - (n - 2 * third), 2 * third, n)]
    for at, lo, hi in spots:
        x[at: at + hi - lo] = a["x"][lo:hi]
    xd = x.to("cuda:0")
    with torch.no_grad():
        lp = flow.log_prob(xd)
        z = flow.backward(xd)
        xr = flow._forward(z)
    torch.cuda.synchronize()
    assert lp.shape == (rows,) and torch.isfinite(lp).all() and torch.isfinite(z).all()
    for at, lo, hi in spots:
        sl = slice(at, at + hi - lo)
        assert _rel(lp[sl], a["log_prob64"][lo:hi]) < 1e-5 and _rel(lp[sl], a["log_prob32"][lo:hi]) < 1e-5, (name, at)
        s = max(1.0, a["backward64"][lo:hi].abs().max().item())
        assert (z[sl].cpu().double() - a["backward64"][lo:hi]).abs().max().item() < 2e-5 * s, (name, at)
    # whole batch: one constant, and the round trip
    base_lp = torch.distributions.Laplace(0.0, 1.0).log_prob(z.double()).flatten(1).sum(-1)
    const = lp.double() - base_lp
    assert (const + float(a["total_ladj64"])).abs().max().item() < 1e-5 * base_lp.abs().max().item()
    # (the round trip passes every layer twice in fp32: the bound grows with the depth -- 2 blocks: 2e-5, the CIFAR
    #  configuration's 10 blocks: 1e-4)
    depth = sum(1 for l in flow.layers if type(l).__name__ == "MaskedCoupling")
    assert (xr - xd).abs().max().item() < 1e-5 * max(2, depth) * max(1.0, xd.abs().max().item())
    # a second call on the same rows is bit-identical (no dependence on the groups' walk order)
    with torch.no_grad():
        assert torch.equal(flow.log_prob(xd), lp)


@pytest.mark.gpu
@pytest.mark.parametrize("cin,cout,ks", [(16, 32, 3), (32, 32, 3), (32, 64, 1), (32, 16, 3)])
def test_conv2d_same_kernel_full_batch(cin, cout, ks):
    """usf_conv2d_same_f32 on the four convolution shapes of the MNIST configuration's conditioner at 65 536 samples
    (7 x 7 pixels): rows sampled at the head, the middle, the tail and at random against F.conv2d in fp64, every
    output finite, and the result independent of the launch (two calls bit-equal)"""
    import torch.nn.functional as F
    from usflows_amd import _ext
    _ext.load()
    B, H, W = FULL_ROWS, 7, 7
    g = torch.Generator().manual_seed(cin * 7 + cout + ks)
    x = torch.randn(B, cin, H, W, generator=g) * 2
    w = torch.randn(cout, cin, ks, ks, generator=g) / (cin * ks * ks) ** 0.5
    b = torch.randn(cout, generator=g)
    xd = x.to("cuda:0")
    planes = _ext.conv2d_weight_planes(w.to("cuda:0"))
    got = _ext.conv2d_same(xd, planes, cout, ks, bias=b.to("cuda:0"), in_act=_ext.ACT_LEAKY_RELU, in_slope=0.0)
    again = _ext.conv2d_same(xd, planes, cout, ks, bias=b.to("cuda:0"), in_act=_ext.ACT_LEAKY_RELU, in_slope=0.0)
    torch.cuda.synchronize()
    assert got.shape == (B, cout, H, W) and torch.isfinite(got).all() and torch.equal(got, again)
    rows = torch.unique(torch.cat([torch.arange(0, 40), torch.arange(B // 2 - 20, B // 2 + 20), torch.arange(B - 40, B),
                                   torch.randint(0, B, (200,), generator=g)]))
    ref = F.conv2d(F.relu(x[rows].double()), w.double(), b.double(), padding=ks // 2)
    err = (got[rows.to("cuda:0")].cpu().double() - ref).abs().max().item()
    assert err < 3e-6 * max(1.0, ref.abs().max().item()), err


@pytest.mark.gpu
@pytest.mark.parametrize("B,cin,cout,H,W", [(3, 32, 16, 7, 7), (4099, 32, 16, 7, 7), (65536, 32, 16, 7, 7), (130, 16, 32, 8, 8)])
def test_conv2d_with_masked_residual_equals_the_two_passes(B, cin, cout, H, W):
    """usf_conv2d_same_res_f32 (the conditioner's last convolution with MaskedCoupling's residual x +- (1 - mask) t in its
    output stream) against usf_conv2d_same_f32 followed by usf_masked_residual_f32: the same arithmetic, bit for bit; and
    shapes the fused form does not serve are refused with the documented code (the caller then runs the two passes)"""
    from usflows_amd import _ext
    _ext.load()
    g = torch.Generator().manual_seed(B + cin + cout)
    x = (torch.randn(B, cin, H, W, generator=g) * 2).to("cuda:0")
    rx = torch.randn(B, cout, H, W, generator=g).to("cuda:0")
    w = torch.randn(cout, cin, 3, 3, generator=g) / (cin * 9) ** 0.5
    b = torch.randn(cout, generator=g).to("cuda:0")
    om = (torch.rand(cout * H * W, generator=g) > 0.5).float().to("cuda:0")
    planes = _ext.conv2d_weight_planes(w.to("cuda:0"))
    for sign in (1.0, -1.0):
        fused = _ext.conv2d_same_res(x, planes, cout, 3, rx, om, sign, bias=b, in_act=_ext.ACT_LEAKY_RELU, in_slope=0.0)
        assert fused is not None
        t = _ext.conv2d_same(x, planes, cout, 3, bias=b, in_act=_ext.ACT_LEAKY_RELU, in_slope=0.0)
        two = _ext.masked_residual(rx, t, om, sign)
        torch.cuda.synchronize()
        assert torch.equal(fused, two)
    # 48 output channels (the CIFAR configuration's last convolution; round 3: the wave-specialised kernel serves them)
    w48 = (torch.randn(48, cin, 3, 3, generator=g) / (cin * 9) ** 0.5).to("cuda:0")
    p48 = _ext.conv2d_weight_planes(w48)
    rx48 = torch.randn(B, 48, H, W, generator=g).to("cuda:0")
    om48 = (torch.rand(48 * H * W, generator=g) > 0.5).float().to("cuda:0")
    fused = _ext.conv2d_same_res(x, p48, 48, 3, rx48, om48, -1.0)
    served = _ext.conv2d_same_variant("res", B, cin, 48, H, W, 3)["kernel"]       # (the launch path's own planner, for this device)
    assert served == 3                                    # these shapes: the wave-specialised kernel, on any number of compute units
    assert (fused is not None) == (served != 0)
    if served:
        assert torch.equal(fused, _ext.masked_residual(rx48, _ext.conv2d_same(x, p48, 48, 3), om48, -1.0))
    # a 1 x 1 kernel: not served by the fused form
    w1 = torch.randn(cout, cin, 1, 1, generator=g).to("cuda:0")
    assert _ext.conv2d_same_res(x, _ext.conv2d_weight_planes(w1), cout, 1, rx, om, 1.0) is None


@pytest.mark.gpu
def test_convnet_spatial_conditioner_runs_on_the_image_kernels(monkeypatch):
    """the reference's generic ``ConvNet`` with 2-D ``in_dims`` (networks.py:312-371) as a MaskedCoupling conditioner: the same
    device passes as ConvNet2D in inference and training -- against the mirror's own torch formulation on the CPU in fp64 (which
    tests/test_mirror_vs_live_reference.py holds bit for bit against the real reference)"""
    import copy
    from usflows_amd import _ext
    DEV = "cuda:0"
    from usflows_amd.flows import USFlow
    from usflows_amd.networks import ConvNet
    from image_synth import synth_image_params_
    dims = [16, 7, 7]
    flow = USFlow(torch.distributions.Laplace(torch.zeros(dims), torch.ones(dims)), dims, 2, ConvNet,
                  dict(in_dims=dims, c_hidden=[32, 32]), householder=0, affine_conjugation=True)
    synth_image_params_(flow, 71)
    x = torch.rand(40, *dims, generator=torch.Generator().manual_seed(4))
    f64 = copy.deepcopy(flow).double()
    for l in f64.layers:
        if torch.is_tensor(getattr(l, "mask", None)):
            l.mask = l.mask.double()
    from usflows_amd.distributions import Independent
    f64.base_distribution = Independent(torch.distributions.Laplace(torch.zeros(dims).double(), torch.ones(dims).double()), 3)
    torch.set_default_dtype(torch.float64)
    try:
        lp64 = f64.log_prob(x.double())
        (-lp64.mean()).backward()
    finally:
        torch.set_default_dtype(torch.float32)
    dev = flow.to(DEV)
    convs, wg = [], []
    real_c, real_w = _ext.conv2d_same, _ext.conv_wgrad
    monkeypatch.setattr(_ext, "conv2d_same", lambda *a_, **k_: (convs.append(1), real_c(*a_, **k_))[1])
    monkeypatch.setattr(_ext, "conv_wgrad", lambda *a_, **k_: (wg.append(1), real_w(*a_, **k_))[1])
    with torch.no_grad():
        lp = dev.log_prob(x.to(DEV))
    assert len(convs) > 0, "the convolutions did not run on usf_conv2d_same_f32"
    assert ((lp.double().cpu() - lp64.detach()).abs() / lp64.detach().abs()).max().item() < 1e-5
    lpg = dev.log_prob(x.to(DEV))
    (-lpg.mean()).backward()
    assert len(wg) > 0, "the weight gradients did not come from usf_conv_wgrad_f32"
    ref = dict(f64.named_parameters())
    for k, p in dev.named_parameters():
        if ref[k].grad is None:
            continue
        s = max(ref[k].grad.abs().max().item(), 1e-30)
        assert (p.grad.double().cpu() - ref[k].grad).abs().max().item() <= 5e-5 * s, k
