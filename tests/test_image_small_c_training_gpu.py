"""Image flows whose affine blocks have 4 or 12 channels (space-to-depth by 2 of a 1- or 3-channel image) train on the device:
every affine layer's backward is ONE usf_channel_affine_bwd_f32 launch (knob ``affine_small_c``) and, above 64 pixels, the gated
conditioner layers take the fused tail (knob ``gated_tail_wide``) -- against the real reference's fp64 gradients and its own SGD
run (tests/golden/wide/, made by tests/golden/make_golden_image_wide.py).  With either knob off the flow takes the route it took
before and gives the same gradients.  The knobs are set here, whatever their defaults are."""
import os

import numpy as np
import pytest
import torch

from golden_util import GOLDEN_DIR, grads_close, load_image_case
from usflows_amd import _ext, image_training
from usflows_amd.config import config
from usflows_amd.transforms import BlockAffineTransform

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CASE_A, CASE_B = "wide/image_a_c4_14x14_k2_gated_ln_hh1_conj", "wide/image_b_c12_16x16_k2_plain_channelmask"
FIT = "fit_a_c4_14x14_k2_gated_ln_hh1_conj"


def _knobs(m, small_c=True, tail_wide=True):
    m.setattr(config, "affine_small_c", small_c)
    m.setattr(config, "gated_tail_wide", tail_wide)


class _Spies:
    """counts of the calls that tell the routes apart"""

    def __init__(self, m, flow=None):
        self.n = dict(affine_bwd=0, affine_fwd=0, tail_bwd=0, wgrad_cc=0, torch_conv=0)
        self.tail_pixels = []
        n = self.n

        def wrap(name, key, seen=None):
            real = getattr(_ext, name)

            def f(*a, **k):
                if seen is None or seen(*a, **k):
                    n[key] += 1
                return real(*a, **k)
            m.setattr(_ext, name, f)

        wrap("channel_affine_bwd", "affine_bwd")
        wrap("channel_affine", "affine_fwd")
        wrap("gated_tail_bwd", "tail_bwd", lambda h, x, *a, **k: self.tail_pixels.append(x.shape[2] * x.shape[3]) or True)
        # a kernel-1 weight gradient from C to C channels: the route an affine block took before (C = 4, 12: no conditioner
        # convolution of these flows has that shape)
        square = lambda x, dy, ks, *a, **k: ks == 1 and x.shape[1] == dy.shape[1] and x.shape[1] <= 12
        wrap("conv_wgrad", "wgrad_cc", square)
        wrap("conv_wgrad_wide", "wgrad_cc", square)
        if flow is not None:
            for blk in (b for b in flow.modules() if isinstance(b, BlockAffineTransform)):
                real = blk.global_transform

                def g(*a, _real=real, **k):
                    n["torch_conv"] += 1
                    return _real(*a, **k)
                m.setattr(blk, "global_transform", g)


def _run(name, m):
    flow, a = load_image_case(name, device=DEV)
    spies = _Spies(m, flow)
    x = a["x"].to(DEV)
    lp = flow.log_prob(x)
    n_fwd = spies.n["affine_fwd"]
    loss = -lp.mean()
    loss.backward()
    torch.cuda.synchronize()
    g_ref = {k[2:]: v for k, v in a.items() if k.startswith("g/")}
    return flow, a, spies, n_fwd, lp.detach(), float(loss.detach()), g_ref


@pytest.mark.parametrize("name", [CASE_A, CASE_B])
def test_every_affine_backward_is_one_launch_and_the_gradients_match_the_reference(name, monkeypatch):
    _knobs(monkeypatch)
    flow, a, spies, n_fwd, lp, loss, g_ref = _run(name, monkeypatch)
    n = spies.n
    n_blocks = sum(1 for b in flow.modules() if isinstance(b, BlockAffineTransform))
    assert n_blocks > 0 and n_fwd > 0, "the flow has no affine layer on the device path"
    # every differentiable channel-affine pass of the forward took its backward from the fused kernel: no separate data-gradient
    # pass (usf_channel_affine_f32 after the forward), no matrix-core weight gradient, no F.conv2d of an affine block
    assert n["affine_bwd"] == n_fwd, n
    assert n["affine_fwd"] == n_fwd and n["wgrad_cc"] == 0 and n["torch_conv"] == 0, n
    if name == CASE_A:
        assert n["tail_bwd"] > 0 and all(p == 196 for p in spies.tail_pixels), (n, spies.tail_pixels)
    ref = a["log_prob64"]
    assert float((lp.cpu().double() - ref).abs().max()) <= 1e-5 * float(ref.abs().max())
    assert abs(loss - float(a["loss"])) < 1e-5 * abs(float(a["loss"]))
    grads_close(dict(flow.named_parameters()), g_ref)


@pytest.mark.parametrize("name", [CASE_A, CASE_B])
def test_affine_small_c_off_restores_the_torch_route(name, monkeypatch):
    _knobs(monkeypatch, small_c=False)
    flow, a, spies, n_fwd, lp, loss, g_ref = _run(name, monkeypatch)
    assert spies.n["affine_bwd"] == 0 and n_fwd == 0 and spies.n["torch_conv"] > 0, spies.n
    assert abs(loss - float(a["loss"])) < 1e-5 * abs(float(a["loss"]))
    grads_close(dict(flow.named_parameters()), g_ref)


def test_gated_tail_wide_off_restores_the_two_pass_tail(monkeypatch):
    _knobs(monkeypatch, tail_wide=False)
    flow, a, spies, n_fwd, lp, loss, g_ref = _run(CASE_A, monkeypatch)
    assert spies.n["tail_bwd"] == 0 and spies.n["affine_bwd"] == n_fwd > 0, spies.n
    assert abs(loss - float(a["loss"])) < 1e-5 * abs(float(a["loss"]))
    grads_close(dict(flow.named_parameters()), g_ref)


@pytest.mark.parametrize("name", [CASE_A, CASE_B])
def test_two_backward_passes_give_the_same_bits_for_the_affine_parameters(name, monkeypatch):
    _knobs(monkeypatch)
    runs = []
    for _ in range(2):
        flow = _run(name, monkeypatch)[0]
        own = {id(p) for b in flow.modules() if isinstance(b, BlockAffineTransform) for p in b.parameters()}
        runs.append({k: p.grad.clone() for k, p in flow.named_parameters() if id(p) in own and p.grad is not None})
    assert len(runs[0]) >= 3 and runs[0].keys() == runs[1].keys()
    for k in runs[0]:
        assert torch.equal(runs[0][k], runs[1][k]), k


def test_the_channel_affine_function_routes_by_channel_count(monkeypatch):
    """image_training.channel_affine_train_ok: C <= 12 at any pixel count on the fused kernel; 16 / 32 / 48 / 64 as ever; any other
    C at 65 .. 256 pixels on usf_conv_wgrad_wide_f32 + usf_channel_affine_f32, declined up to 64 pixels -- and ChannelAffine's
    gradients at one shape of each route against fp64"""
    _knobs(monkeypatch)
    ok = lambda C, H, W, B=8: image_training.channel_affine_train_ok(torch.empty(B, C, H, W, device=DEV), C)
    assert all(ok(C, H, W) for C in (1, 3, 4, 12) for H, W in ((1, 1), (7, 7), (14, 14), (16, 16), (20, 20)))
    assert all(ok(C, H, W) for C in (16, 32, 48, 64) for H, W in ((7, 7), (9, 9), (16, 16)))
    assert all(ok(C, H, W) for C in (13, 20, 24, 40, 63) for H, W in ((9, 9), (14, 14), (16, 16)))
    assert not any(ok(C, H, W) for C in (13, 20, 24, 40, 63) for H, W in ((7, 7), (8, 8), (17, 17)))
    assert not ok(65, 9, 9) and not ok(16, 17, 17)
    monkeypatch.setattr(config, "affine_small_c", False)
    assert not any(ok(C, H, W) for C in (1, 4, 12) for H, W in ((7, 7), (14, 14)))
    assert ok(16, 7, 7) and ok(20, 9, 9)
    monkeypatch.setattr(config, "affine_small_c", True)
    for C, H, pre_sub in ((4, 14, False), (12, 16, True), (5, 7, True), (20, 9, False), (20, 9, True)):
        g = torch.Generator().manual_seed(C + H)
        x, W, b = torch.randn(6, C, H, H, generator=g), torch.randn(C, C, generator=g), torch.randn(C, generator=g)
        dy = torch.randn(6, C, H, H, generator=g)
        xd, Wd, bd = (t.double().requires_grad_() for t in (x, W, b))
        v = xd - bd.view(1, C, 1, 1) if pre_sub else xd
        yd = torch.einsum("ck,bkhw->bchw", Wd, v) + (0 if pre_sub else bd.view(1, C, 1, 1))
        yd.backward(dy.double())
        xg, Wg, bg = (t.to(DEV).requires_grad_() for t in (x, W, b))
        y = image_training.ChannelAffine.apply(xg, Wg, bg, pre_sub)
        y.backward(dy.to(DEV))
        for got, ref in ((y.detach(), yd.detach()), (xg.grad, xd.grad), (Wg.grad, Wd.grad), (bg.grad, bd.grad)):
            assert float((got.cpu().double() - ref).abs().max()) <= 1e-5 * float(ref.abs().max()), (C, H, pre_sub)


def test_fit_eager_and_replayed_matches_the_reference_run(monkeypatch):
    """Flow.fit of case (a) against the reference's own 2-epoch SGD run with the bounds of
    test_image_wide_training_gpu.py::test_fit_eager_and_replayed_matches_the_reference_run (losses 2e-4, parameters 2e-3 of the
    tensor's largest entry, every tensor's total update 1e-2 of the update's largest entry), eager and replayed, on the new
    routes; replayed: every step behind the eager ones is a graph replay (the count tools/bench_fit_optim.py reads)"""
    _knobs(monkeypatch)
    z = np.load(os.path.join(GOLDEN_DIR, "wide", FIT + ".npz"), allow_pickle=False)
    data, losses_ref, lr = torch.from_numpy(z["data"]), [float(v) for v in z["losses"]], float(z["lr"])
    sd_ref = {k[3:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("sd/")}
    steps = 2 * (data.shape[0] // 32)
    for graph in ("0", "1"):
        monkeypatch.setenv("USFLOWS_AMD_TRAIN_GRAPH", graph)
        flow, _ = load_image_case(CASE_A, device=DEV)
        sd0 = {k: v.detach().cpu().double().clone() for k, v in flow.state_dict().items()}
        with monkeypatch.context() as m:
            spies = _Spies(m, flow)
            ds = torch.utils.data.TensorDataset(data, torch.zeros(data.shape[0]))
            np.random.seed(5)
            losses = flow.fit(ds, optim=torch.optim.SGD, optim_params=dict(lr=lr), batch_size=32, shuffle=True,
                              device=torch.device(DEV), epochs=2)
        n = spies.n
        assert n["affine_bwd"] > 0 and n["tail_bwd"] > 0 and n["torch_conv"] == 0 and n["wgrad_cc"] == 0, (graph, n)
        replays = (flow.__dict__.get("_train_graph_state") or {}).get("replays", 0)
        assert replays == (steps - flow._TRAIN_GRAPH_EAGER_STEPS if graph == "1" else 0), (graph, replays, steps)
        sd = flow.state_dict()
        worst, worst_up, moved = (0.0, ""), (0.0, ""), 0
        for k, v in sd_ref.items():
            d = (sd[k].cpu().double() - v.double()).abs().max().item()
            worst = max(worst, (d / max(v.abs().max().item(), 1e-3), k))
            up = (v.double() - sd0[k]).abs().max().item()
            if up > 0:
                moved += 1
                worst_up = max(worst_up, (d / up, k))
        print(f"graph {graph}: losses {[float(l) for l in losses]} (reference {losses_ref}); replays {replays} of {steps} steps; "
              f"worst parameter {worst}; worst update {worst_up}")
        for l, r in zip(losses, losses_ref):
            assert abs(float(l) - r) < 2e-4 * abs(r), (graph, losses, losses_ref)
        assert worst[0] < 2e-3, (graph, worst)
        assert moved >= 30 and worst_up[0] < 1e-2, (graph, worst_up)
