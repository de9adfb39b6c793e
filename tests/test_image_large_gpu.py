"""Image-shaped flows whose feature maps have more than 256 pixels ([1, 28, 28], [3, 32, 32], [2, 17, 17]) on the device, with
the knob ``conv_band`` set here (the tests do not depend on its default): against the REAL reference's goldens
(tests/golden/image_large/*.npz, made by tests/golden/make_golden_image_large.py) at the project's bound, 1e-5 relative to the
reference's fp64 run; every Conv2d of every conditioner on the row-banded kernel and no torch convolution; the same values with
the knob off; the hipGraph replay of 100 rows; sampling; what stays on torch (64 hidden channels at kernel 3; training)."""
import json
import os
import warnings

import numpy as np
import pytest
import torch

from cond_image_cases import run_layers
from golden_util import build_image_radial_flow

DEV = "cuda:0"
pytestmark = pytest.mark.gpu
DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "image_large")
MNIST, CIFAR, COND = "imagelarge_mnist_c1_28x28", "imagelarge_cifar_c3_32x32", "imagelarge_cond_c2_17x17"


def load_case(name, device=DEV):
    """(mirror USFlow with the parameters of tests/image_synth.py, arrays) of a case, built as the generator built the reference's"""
    from image_synth import synth_image_params_
    from usflows_amd import networks
    from usflows_amd.flows import USFlow
    z = np.load(os.path.join(DIR, name + ".npz"), allow_pickle=False)
    d = json.loads(str(z["spec"]))
    dims = d["in_dims"]
    arrays = {k: torch.from_numpy(z[k]) for k in z.files if k != "spec"}
    if d.get("base") == "lognormal":
        return build_image_radial_flow(d, {}, device), arrays
    torch.manual_seed(d["seed"])
    base = torch.distributions.Laplace(torch.zeros(dims), torch.ones(dims))
    flow = USFlow(base, dims, d["coupling_blocks"], getattr(networks, d["cond_cls"]), dict(d["cond_args"]), householder=d["householder"],
                  affine_conjugation=d["affine_conjugation"], soft_training=d["cond_cls"].startswith("Cond"))
    synth_image_params_(flow, d["seed"])
    return flow.to(device), arrays


@pytest.fixture
def band(monkeypatch):
    from usflows_amd.config import config
    monkeypatch.setattr(config, "conv_band", True)
    return config


def _rel(got, want):
    return ((got.cpu().double() - want).abs().max() / want.abs().max()).item()


class _Launches:
    """names of the library launches and of the torch convolutions a block issues"""

    def __init__(self, monkeypatch):
        from torch.utils._python_dispatch import TorchDispatchMode
        from usflows_amd import _ext
        self.names, self.aten = [], []
        real = _ext._launch
        monkeypatch.setattr(_ext, "_launch", lambda name, *a, **k: (self.names.append(name), real(name, *a, **k))[1])
        outer = self

        class Mode(TorchDispatchMode):
            def __torch_dispatch__(self, func, types, args=(), kwargs=None):
                if "conv" in str(func):
                    outer.aten.append(str(func))
                return func(*args, **(kwargs or {}))
        self.mode = Mode

    def count(self, name):
        return sum(1 for n in self.names if n == name)


def _convs(flow):
    """(3 x 3 convolutions, 1 x 1 convolutions) of all conditioners"""
    cs = list({id(m): m for m in flow.modules() if isinstance(m, torch.nn.Conv2d)}.values())
    return [c for c in cs if c.kernel_size == (3, 3)], [c for c in cs if c.kernel_size == (1, 1)]


@pytest.mark.parametrize("name", [MNIST, CIFAR])
def test_large_image_flow_matches_the_reference(name, band):
    flow, a = load_case(name)
    x, zin = a["x"].to(DEV), a["zin"].to(DEV)
    with warnings.catch_warnings():
        warnings.simplefilter("error", RuntimeWarning)
        with torch.no_grad():
            assert _rel(flow.log_prob(x), a["log_prob64"]) <= 1e-5
            assert _rel(flow.log_prob(x), a["log_prob32"].double()) <= 1e-5
            assert _rel(flow.backward(x), a["backward64"]) <= 1e-5
            assert _rel(flow._forward(zin), a["forward64"]) <= 1e-5


def test_large_conditional_flow_matches_the_reference(band, monkeypatch):
    flow, a = load_case(COND)
    x, zin, ctx = a["x"].to(DEV), a["zin"].to(DEV), a["ctx"].to(DEV)
    rec = _Launches(monkeypatch)
    with torch.no_grad():
        assert _rel(flow.log_prob(x, ctx), a["log_prob64_ctx"]) <= 1e-5
        assert _rel(flow.log_prob(x), a["log_prob64_noctx"]) <= 1e-5
        with rec.mode():
            assert _rel(run_layers(flow, x, ctx, True), a["backward64_ctx"]) <= 1e-5
            assert _rel(run_layers(flow, zin, ctx, False), a["forward64_ctx"]) <= 1e-5
            assert _rel(run_layers(flow, x, torch.zeros_like(ctx), True), a["backward64_noctx"]) <= 1e-5
    k3, k1 = _convs(flow)
    assert rec.aten == [] and rec.count("usf_conv2d_same_ctx_f32") == 0
    assert rec.count("usf_conv2d_same_band_f32") >= 3 * len(k3 + k1) > 0


def test_every_conv2d_of_every_conditioner_is_one_band_launch(band, monkeypatch):
    """log_prob of the [1, 28, 28] case: one usf_conv2d_same_band_f32 launch per 3 x 3 Conv2d of every conditioner (GatedConv's 1 x 1
    convolution and its gate are one pass of the per-pixel kernels, as at 7 x 7), no torch convolution.  Fails without the feature"""
    flow, a = load_case(MNIST)
    x = a["x"].to(DEV)
    k3, k1 = _convs(flow)
    assert len(k3) >= 8 and len(k1) >= 4                         # per block: first + 2 gated + last | 2 gate convolutions
    flow.graph_max_rows = 0                                      # (the eager loop: one pass per call, no recording or capture run beside it)
    with torch.no_grad():
        flow.log_prob(x)                                         # (first sighting: the merged-affine probe runs the layers twice more)
    rec = _Launches(monkeypatch)
    with torch.no_grad(), rec.mode():
        lp = flow.log_prob(x)
    assert rec.aten == [], rec.aten
    assert rec.count("usf_conv2d_same_band_f32") == len(k3)
    assert rec.count("usf_pointwise_conv_f32") + rec.count("usf_gated_tail_f32") == len(k1)
    assert _rel(lp, a["log_prob64"]) <= 1e-5
    # the knob off: the same values within the bound, through torch's convolution
    band.conv_band = False
    flow2, _ = load_case(MNIST)
    flow2.graph_max_rows = 0
    with torch.no_grad():
        flow2.log_prob(x)
    rec2 = _Launches(monkeypatch)
    with torch.no_grad(), rec2.mode():
        lp2 = flow2.log_prob(x)
    assert rec2.count("usf_conv2d_same_band_f32") == 0 and len(rec2.aten) >= len(k3)
    assert _rel(lp2, a["log_prob64"]) <= 1e-5 and _rel(lp2, lp.cpu().double()) <= 1e-5


def test_100_rows_replay_as_a_graph_with_the_same_bits(band):
    """the band launch has no op-list id: the recorded list is marked bad, 100 rows are served by the hipGraph replay -- the same
    bits on every call, and again after an in-place parameter change"""
    flow, a = load_case(MNIST)
    x = torch.rand(100, 1, 28, 28, generator=torch.Generator().manual_seed(9)).to(DEV)
    with torch.no_grad():
        flow.graph_max_rows = 0
        eager = flow.log_prob(x)
        flow.graph_max_rows = 256
        outs = [flow.log_prob(x) for _ in range(4)]
        assert all(torch.equal(o, eager) for o in outs)
        assert flow._loop_lists[(tuple(x.shape), DEV)][1] is None, "a pass with a band launch was recorded as an op list"
        assert (tuple(x.shape), DEV) in flow._loop_graphs and not getattr(flow, "_loop_graph_off", False)
        for p in flow.parameters():
            if p.numel() > 1:
                p.mul_(1.0 + 1e-3)
        flow.graph_max_rows = 0
        eager2 = flow.log_prob(x)
        flow.graph_max_rows = 256
        outs = [flow.log_prob(x) for _ in range(4)]
        assert all(torch.equal(o, eager2) for o in outs) and not torch.equal(eager2, eager)


def test_sample_returns_the_philox_latents_and_the_udl_constant_is_flat(band, monkeypatch):
    from usflows_amd import radial
    flow, a = load_case(CIFAR)
    rec = _Launches(monkeypatch)
    with torch.no_grad():
        xs = flow.sample([8], seed=3)
        assert xs.shape == (8, 3, 32, 32) and torch.isfinite(xs).all()
        z = flow.backward(xs)
        want = radial.sample(flow.base_distribution, 8, 3, 0, 0).reshape(8, 3, 32, 32)
        assert _rel(z, want.cpu().double()) <= 1e-5
        lp = flow.log_prob(xs) - flow.base_distribution.log_prob(z)
        assert (lp - lp.mean()).abs().max().item() < 1e-4 * abs(lp.mean().item())
    assert rec.count("usf_conv2d_same_band_f32") >= 3 * len(_convs(flow)[0])


def test_64_hidden_channels_at_kernel_3_stay_on_torch(band, monkeypatch):
    """64 -> 64 at 3 x 3 has 224 KB of weight planes: not served; the flow runs through torch's convolution there, with no
    RuntimeWarning other than the project's one about the composite formulation"""
    from image_synth import synth_image_params_
    from usflows_amd.flows import USFlow
    from usflows_amd.networks import ConvNet2D
    dims = [3, 32, 32]
    torch.manual_seed(5)
    flow = USFlow(torch.distributions.Laplace(torch.zeros(dims), torch.ones(dims)), dims, 1, ConvNet2D,
                  dict(c_in=3, c_hidden=64, num_layers=2, kernel_size=3, padding="same", normalize_layers=True, gating=True), householder=1,
                  affine_conjugation=True)
    synth_image_params_(flow, 5)
    flow = flow.to(DEV)
    x = torch.rand(2, *dims, generator=torch.Generator().manual_seed(1)).to(DEV)
    flow.graph_max_rows = 0
    rec = _Launches(monkeypatch)
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        with torch.no_grad():
            flow.log_prob(x)                                     # (first sighting: the merged-affine probe runs the layers twice more)
            del rec.names[:]
            with rec.mode():
                lp = flow.log_prob(x)
    assert torch.isfinite(lp).all() and any("convolution" in f for f in rec.aten)
    from usflows_amd.image_rules import band_conv_ok
    served = [c for c in _convs(flow)[0] if band_conv_ok(c.in_channels, c.out_channels, 32, 32, 3)]
    assert {(c.in_channels, c.out_channels) for c in served} == {(3, 64), (64, 3)}      # 64 -> 64 is not
    assert rec.count("usf_conv2d_same_band_f32") == len(served)
    rw = [w for w in caught if issubclass(w.category, RuntimeWarning)]
    assert len(rw) <= 1 and all("composite formulation" in str(w.message) for w in rw)
    band.conv_band = False
    with torch.no_grad():
        assert _rel(flow.log_prob(x), lp.cpu().double()) <= 1e-5


def test_fit_keeps_torch_autograd(band, monkeypatch):
    """training is out of scope: no weight-gradient kernel serves more than 256 pixels, so the conditioners' train_on_device stays
    False and Flow.fit runs two steps through torch autograd, without a band launch"""
    flow, a = load_case(MNIST)
    x = torch.rand(64, 1, 28, 28, generator=torch.Generator().manual_seed(2))
    cond = next(l for l in flow.layers if type(l).__name__ == "MaskedCoupling")
    nets = [m for m in cond.modules() if hasattr(m, "train_on_device")]
    assert nets and not any(m.train_on_device(x[:32].to(DEV)) for m in nets)
    rec = _Launches(monkeypatch)
    before = [p.detach().clone() for p in flow.parameters()]
    losses = flow.fit(torch.utils.data.TensorDataset(x, torch.zeros(64)), optim=torch.optim.SGD, optim_params=dict(lr=1e-4), batch_size=32,
                      shuffle=False, device=torch.device(DEV), epochs=1)
    assert all(np.isfinite(float(v)) for v in losses)
    assert rec.count("usf_conv2d_same_band_f32") == 0
    assert any(not torch.equal(p.detach(), b) for p, b in zip(flow.parameters(), before))
