"""Image flows with feature maps of 257 .. 4096 pixels ([1, 28, 28], [3, 32, 32]) train on the device under the knob
``train_band`` (set here by monkeypatch; it ships off): ``Flow.log_prob`` under autograd and ``Flow.fit`` against the real
reference's fp64 gradients and its own SGD run (tests/golden/image_large_train/, made by
tests/golden/make_golden_image_large_grads.py).  Forward and data gradient run on usf_conv2d_same_band_f32, the weight gradients
on usf_conv_wgrad_band_f32; with the knob off the flows take the torch autograd route they take today and give the same
gradients.  Beside them the elementwise backward kernels these maps reach, at 784 and 1024 pixels.

Not covered by a flow fixture: affine blocks of 16 .. 64 channels above 256 pixels (they reach the new kernel through
``wgrad_served``; tests/test_conv_wgrad_band_gpu.py holds the kernel itself at such shapes) and ``gated_tail_wide``."""
import json
import os

import numpy as np
import pytest
import torch

from golden_util import GOLDEN_DIR, build_image_radial_flow, grads_close
from usflows_amd import _ext
from usflows_amd.config import config
from usflows_amd.networks import ConvNet2D

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DIR = os.path.join(GOLDEN_DIR, "image_large_train")
MNIST, CIFAR, FIT = "imagelargegrads_mnist_c1_28x28", "imagelargegrads_cifar_c3_32x32", "imagelargefit_mnist_c1_28x28"
WGRAD = "usf_conv_wgrad_band_f32"


def _flow(spec, device=DEV):
    """the mirror's flow with the parameters of tests/image_synth.py, built as the generator built the reference's"""
    from image_synth import synth_image_params_
    from usflows_amd.flows import USFlow
    dims = spec["in_dims"]
    if spec.get("base") == "lognormal":
        return build_image_radial_flow(spec, {}, device)
    torch.manual_seed(spec["seed"])
    flow = USFlow(torch.distributions.Laplace(torch.zeros(dims), torch.ones(dims)), dims, spec["coupling_blocks"], ConvNet2D,
                  dict(spec["cond_args"]), householder=spec["householder"], affine_conjugation=spec["affine_conjugation"])
    synth_image_params_(flow, spec["seed"])
    return flow.to(device)


def load_case(name):
    z = np.load(os.path.join(DIR, name + ".npz"), allow_pickle=False)
    spec = json.loads(str(z["spec"]))
    return _flow(spec), {k: torch.from_numpy(z[k]) for k in z.files if k != "spec"}, spec


class _Launches:
    """names of the library launches and of the torch convolutions a block issues (the recorder of test_image_large_gpu.py)"""

    def __init__(self, monkeypatch):
        from torch.utils._python_dispatch import TorchDispatchMode
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


def _run(name, monkeypatch):
    flow, a, _ = load_case(name)
    x = a["x"].to(DEV)
    nets = [m for m in flow.modules() if isinstance(m, ConvNet2D)]
    assert nets
    served = [m.train_on_device(x) for m in nets]
    rec = _Launches(monkeypatch)
    with rec.mode():
        lp = flow.log_prob(x)
        loss = -lp.mean()
        loss.backward()
    torch.cuda.synchronize()
    g_ref = {k[2:]: v for k, v in a.items() if k.startswith("g/")}
    convs = list({id(m): m for m in flow.modules() if isinstance(m, torch.nn.Conv2d)}.values())
    return flow, a, served, lp.detach(), float(loss.detach()), g_ref, rec, convs


def _split_zero_gradients(g_ref):
    """(gradients held relatively, {name: scale} of those held absolutely).  The Householder vector of a ONE-channel affine block has
    a gradient that is zero analytically (the reflection of a 1-vector is -1 whatever the vector): the reference's fp64 run
    leaves 1e-17 of noise there, which no relative bound can be held to.  Such a tensor -- its fp64 gradient below 2^-40 of the
    largest gradient of the same block's other factors -- is held to 5e-5 of THAT scale instead: a gradient wrongly routed there
    would be of its order"""
    rel, absolute = {}, {}
    for k, g in g_ref.items():
        block = k.rsplit(".transforms.", 1)[0]
        scale = max(float(v.abs().max()) for q, v in g_ref.items() if q != k and q.rsplit(".transforms.", 1)[0] == block) \
            if ".transforms." in k else 0.0
        if scale > 0 and 0 < float(g.abs().max()) < 2.0 ** -40 * scale:     # (an exact zero is held as it is: grads_close asks for a zero)
            absolute[k] = scale
        else:
            rel[k] = g
    return rel, absolute


def _hold(flow, a, lp, loss, g_ref):
    ref = a["log_prob64"]
    print(f"log_prob {float((lp.cpu().double() - ref).abs().max()) / float(ref.abs().max()):.2e}, loss "
          f"{abs(loss - float(a['loss'])) / abs(float(a['loss'])):.2e} (bounds 1e-5)")
    assert float((lp.cpu().double() - ref).abs().max()) <= 1e-5 * float(ref.abs().max())
    assert abs(loss - float(a["loss"])) <= 1e-5 * abs(float(a["loss"]))
    named = dict(flow.named_parameters())
    rel, absolute = _split_zero_gradients(g_ref)
    assert all(k.endswith("vk_householder") and g_ref[k].numel() == 1 for k in absolute), sorted(absolute)
    grads_close(named, rel)
    for k, scale in absolute.items():
        got = float(named[k].grad.abs().max())
        print(f"{k}: analytically zero; device {got:.2e}, the block's gradient scale {scale:.2e}")
        assert got <= 5e-5 * scale, (k, got, scale)


@pytest.mark.parametrize("name", [MNIST, CIFAR])
def test_gradients_match_the_real_reference_on_the_band_kernels(name, monkeypatch):
    monkeypatch.setattr(config, "conv_band", True)
    monkeypatch.setattr(config, "train_band", True)
    flow, a, served, lp, loss, g_ref, rec, convs = _run(name, monkeypatch)
    assert all(served), served
    assert rec.aten == [], rec.aten
    assert len(convs) >= 6 and rec.count(WGRAD) >= len(convs), (rec.count(WGRAD), len(convs))
    assert rec.count("usf_conv2d_same_band_f32") >= len([c for c in convs if c.kernel_size == (3, 3)])
    assert len(g_ref) >= len(list(flow.parameters())) - 2 > 0
    _hold(flow, a, lp, loss, g_ref)


@pytest.mark.parametrize("name", [MNIST, CIFAR])
def test_the_knob_off_keeps_the_torch_route(name, monkeypatch):
    monkeypatch.setattr(config, "conv_band", True)
    assert config.train_band is False
    flow, a, served, lp, loss, g_ref, rec, convs = _run(name, monkeypatch)
    assert not any(served) and rec.count(WGRAD) == 0 and len(rec.aten) > 0
    _hold(flow, a, lp, loss, g_ref)


def test_fit_eager_and_replayed_matches_the_reference_run(monkeypatch):
    """Flow.fit of the [1, 28, 28] case against the reference's own 2-epoch SGD run (64 rows, batch 32, numpy seed 5), eager and
    replayed, with the bounds of test_image_wide_training_gpu.py: losses 2e-4, parameters 2e-3 of the tensor's largest entry,
    every tensor's total update 1e-2 of the update's largest entry (the fixture records the learning rate and the reference's
    own fp32-against-fp64 gap: a tenth of these bounds for losses and parameters, 1.2e-3 for the updates); two replayed runs give
    the same bits"""
    monkeypatch.setattr(config, "conv_band", True)
    monkeypatch.setattr(config, "train_band", True)
    z = np.load(os.path.join(DIR, FIT + ".npz"), allow_pickle=False)
    data, losses_ref, lr = torch.from_numpy(z["data"]), [float(v) for v in z["losses"]], float(z["lr"])
    sd_ref = {k[3:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("sd/")}
    spec = json.loads(str(np.load(os.path.join(DIR, MNIST + ".npz"), allow_pickle=False)["spec"]))
    assert spec["seed"] == int(z["seed"])
    counted = set(json.loads(str(z["update_keys"])))
    assert 30 <= len(counted) < len(sd_ref)
    replayed = []
    for graph in ("0", "1", "1"):
        monkeypatch.setenv("USFLOWS_AMD_TRAIN_GRAPH", graph)
        flow = _flow(spec)
        sd0 = {k: v.detach().cpu().double().clone() for k, v in flow.state_dict().items()}
        with monkeypatch.context() as m:
            rec = _Launches(m)
            ds = torch.utils.data.TensorDataset(data, torch.zeros(data.shape[0]))
            np.random.seed(5)
            losses = flow.fit(ds, optim=torch.optim.SGD, optim_params=dict(lr=lr), batch_size=32, shuffle=True, device=torch.device(DEV),
                              epochs=2)
        assert rec.count(WGRAD) > 0, "Flow.fit did not reach the band weight-gradient kernel"
        sd = {k: v.detach().cpu().clone() for k, v in flow.state_dict().items()}
        if graph == "1":
            replayed.append(([float(l) for l in losses], sd))
        worst, worst_up, moved = (0.0, ""), (0.0, ""), 0
        for k, v in sd_ref.items():
            d = (sd[k].double() - v.double()).abs().max().item()
            worst = max(worst, (d / max(v.abs().max().item(), 1e-3), k))
            up = (v.double() - sd0[k]).abs().max().item()
            if k in counted and up > 0:                                # (the generator's rule: the Householder vectors of a one-channel block do not move)
                moved += 1
                worst_up = max(worst_up, (d / up, k))
        print(f"graph {graph}: losses {[float(l) for l in losses]} (reference {losses_ref}); worst parameter {worst}; worst update {worst_up}")
        for l, r in zip(losses, losses_ref):
            assert abs(float(l) - r) < 2e-4 * abs(r), (graph, losses, losses_ref)
        assert worst[0] < 2e-3, (graph, worst)
        assert moved >= 30 and worst_up[0] < 1e-2, (graph, worst_up)
    assert replayed[0][0] == replayed[1][0] and all(torch.equal(replayed[0][1][k], replayed[1][1][k]) for k in replayed[0][1])


@pytest.mark.parametrize("P", [784, 1024])
@pytest.mark.parametrize("B", [1, 3])
def test_layernorm_backward_at_784_and_1024_pixels_vs_fp64(P, B):
    """usf_layernorm_channels_bwd_f32 (LayerNormCh's backward) indexes pixels as b * P + p with no bound on P: held here at the
    pixel counts the flows above bring, C = 32"""
    C = 32
    g = torch.Generator().manual_seed(P + B)
    x = torch.randn(B, C, P, generator=g)
    x = x + torch.where(x.abs() < 1e-3, 2e-3 * torch.sign(x), torch.zeros(()))
    dy, gamma, beta = torch.randn(B, C, P, generator=g), 1 + 0.2 * torch.randn(C, generator=g), torch.randn(C, generator=g)
    eps = 1e-5
    xd = x.double().requires_grad_()
    gd, bd = gamma.double().requires_grad_(), beta.double().requires_grad_()
    a = torch.relu(xd)
    mean = a.mean(1, keepdim=True)
    y = (a - mean) / torch.sqrt(((a - mean) ** 2).mean(1, keepdim=True) + eps) * gd.view(1, C, 1) + bd.view(1, C, 1)
    y.backward(dy.double())
    dx, dg, dbt = _ext.layernorm_channels_bwd(x.to(DEV), dy.to(DEV), gamma.to(DEV), eps, _ext.ACT_LEAKY_RELU, 0.0)
    for got, ref in ((dx, xd.grad), (dg, gd.grad), (dbt, bd.grad)):
        assert float((got.cpu().double() - ref).abs().max()) <= 1e-5 * float(ref.abs().max())


@pytest.mark.parametrize("P", [784, 1024])
@pytest.mark.parametrize("C", [1, 3])
def test_channel_affine_backward_at_784_and_1024_pixels_vs_fp64(C, P):
    """usf_channel_affine_bwd_f32 at the affine blocks of the two flows (C = 1 and 3), B = 3, both forms, at that kernel's own
    bound: 2e-6 of max|ref|"""
    B = 3
    g = torch.Generator().manual_seed(100 * C + P)
    x, dy = torch.randn(B, C, P, generator=g), torch.randn(B, C, P, generator=g)
    W, b = torch.randn(C, C, generator=g) + 2 * torch.eye(C), torch.randn(C, generator=g)
    for pre_sub in (False, True):
        xin = x.double() - b.double().view(1, C, 1) if pre_sub else x.double()
        ref = (torch.einsum("oi,bop->bip", W.double(), dy.double()), torch.einsum("bop,bip->oi", dy.double(), xin), dy.double().sum((0, 2)))
        got = _ext.channel_affine_bwd(x.to(DEV), dy.to(DEV), W.to(DEV), pre_sub=b.to(DEV) if pre_sub else None)
        assert got is not None
        for gt, rf, what in zip(got, ref, ("dx", "dW", "db")):
            err, scale = float((gt.cpu().double() - rf).abs().max()), float(rf.abs().max())
            print(f"C {C} P {P} pre_sub {pre_sub} {what}: {err / scale:.2e} of max|ref|")
            assert err <= 2e-6 * scale, (C, P, pre_sub, what, err / scale)
