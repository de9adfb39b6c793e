"""Image flows with feature maps of 65 .. 256 pixels train on the device: ``Flow.log_prob`` under autograd and ``Flow.fit`` against
the real reference's fp64 gradients and its own SGD run (tests/golden/wide/, made by tests/golden/make_golden_image_wide.py).
The weight gradients of these shapes come from usf_conv_wgrad_wide_f32; with the knob ``wgrad_wide`` off the flows take the
torch autograd route they took before and give the same gradients."""
import os

import numpy as np
import pytest
import torch

from golden_util import GOLDEN_DIR, grads_close, load_image_case
from usflows_amd import _ext
from usflows_amd.config import config
from usflows_amd.networks import ConvNet2D

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CASES = ["wide/image_a_c4_14x14_k2_gated_ln_hh1_conj", "wide/image_b_c12_16x16_k2_plain_channelmask",
         "wide/image_c_c16_9x9_k2_gated_ln_hh1_conj"]
FIT = "fit_a_c4_14x14_k2_gated_ln_hh1_conj"


def _count_wide(monkeypatch):
    calls = []
    real = _ext.conv_wgrad_wide
    monkeypatch.setattr(_ext, "conv_wgrad_wide", lambda *a, **k: (calls.append(a[0].shape), real(*a, **k))[1])
    return calls


def _run(name):
    flow, a = load_image_case(name, device=DEV)
    x = a["x"].to(DEV)
    nets = [m for m in flow.modules() if isinstance(m, ConvNet2D)]
    assert nets
    served = [m.train_on_device(x) for m in nets]
    lp = flow.log_prob(x)
    loss = -lp.mean()
    loss.backward()
    g_ref = {k[2:]: v for k, v in a.items() if k.startswith("g/")}
    return flow, a, served, lp.detach(), float(loss.detach()), g_ref


@pytest.mark.parametrize("name", CASES)
def test_gradients_match_the_real_reference_on_the_wide_kernel(name, monkeypatch):
    assert config.wgrad_wide
    calls = _count_wide(monkeypatch)
    flow, a, served, lp, loss, g_ref = _run(name)
    assert all(served), served
    assert len(calls) > 0 and all(s[2] * s[3] > 64 for s in calls)
    if name == CASES[2]:
        assert any(s[1] == 16 and s[2:] == (9, 9) for s in calls)          # the affine blocks' ChannelAffine at C = 16
    ref = a["log_prob64"]
    assert float((lp.cpu().double() - ref).abs().max()) <= 1e-5 * float(ref.abs().max())
    assert abs(loss - float(a["loss"])) < 1e-5 * abs(float(a["loss"]))
    grads_close(dict(flow.named_parameters()), g_ref)


@pytest.mark.parametrize("name", CASES)
def test_the_knob_restores_the_torch_route(name, monkeypatch):
    monkeypatch.setattr(config, "wgrad_wide", False)
    calls = _count_wide(monkeypatch)
    flow, a, served, lp, loss, g_ref = _run(name)
    assert not any(served) and not calls
    assert abs(loss - float(a["loss"])) < 1e-5 * abs(float(a["loss"]))
    grads_close(dict(flow.named_parameters()), g_ref)


def test_fit_eager_and_replayed_matches_the_reference_run(monkeypatch):
    """Flow.fit of case (a) against the reference's own 2-epoch SGD run (96 rows, batch 32, numpy seed 5), eager and replayed,
    with the bounds of test_image_flow_fit_on_device_matches_reference_run: losses 2e-4, parameters 2e-3 of the tensor's largest
    entry.  The run's learning rate is the fixture's (1e-5; make_golden_image_wide.py says why 1e-3 pins nothing for this flow),
    at which some tensors move by less than those 2e-3 in six steps -- so every tensor's total UPDATE is held too, to 1e-2 of
    the update's largest entry: the reference's fp32 run is up to 1.6e-3 from its own fp64 run in that unit over the candidate
    seeds (fp32 rounding of updates of 1e-4 to values of size one), and six times that is allowed for another fp32 order.
    A step that is skipped, doubled or scaled wrongly, or a gradient that is off by a few percent, misses it."""
    z = np.load(os.path.join(GOLDEN_DIR, "wide", FIT + ".npz"), allow_pickle=False)
    data, losses_ref, lr = torch.from_numpy(z["data"]), [float(v) for v in z["losses"]], float(z["lr"])
    sd_ref = {k[3:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("sd/")}
    for graph in ("0", "1"):
        monkeypatch.setenv("USFLOWS_AMD_TRAIN_GRAPH", graph)
        flow, _ = load_image_case(CASES[0], device=DEV)
        sd0 = {k: v.detach().cpu().double().clone() for k, v in flow.state_dict().items()}
        with monkeypatch.context() as m:
            calls = _count_wide(m)
            ds = torch.utils.data.TensorDataset(data, torch.zeros(data.shape[0]))
            np.random.seed(5)
            losses = flow.fit(ds, optim=torch.optim.SGD, optim_params=dict(lr=lr), batch_size=32, shuffle=True,
                              device=torch.device(DEV), epochs=2)
        assert len(calls) > 0, "Flow.fit did not reach the wide weight-gradient kernel"
        sd = flow.state_dict()
        worst, worst_up, moved = (0.0, ""), (0.0, ""), 0
        for k, v in sd_ref.items():
            d = (sd[k].cpu().double() - v.double()).abs().max().item()
            worst = max(worst, (d / max(v.abs().max().item(), 1e-3), k))
            up = (v.double() - sd0[k]).abs().max().item()
            if up > 0:
                moved += 1
                worst_up = max(worst_up, (d / up, k))
        print(f"graph {graph}: losses {[float(l) for l in losses]} (reference {losses_ref}); worst parameter {worst}; worst update {worst_up}")
        for l, r in zip(losses, losses_ref):
            assert abs(float(l) - r) < 2e-4 * abs(r), (graph, losses, losses_ref)
        assert worst[0] < 2e-3, (graph, worst)
        assert moved >= 30 and worst_up[0] < 1e-2, (graph, worst_up)


@pytest.mark.parametrize("P", [81, 196, 256])
@pytest.mark.parametrize("B", [3, 33])
def test_layernorm_backward_above_64_pixels_vs_fp64(P, B):
    """usf_layernorm_channels_bwd_f32 is routed above 64 pixels with these flows (its kernels index pixels as b * P + p with no
    bound on P; the gated tail is not: image_training.gated_tail_ok declines above 64 pixels)"""
    C = 16
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
