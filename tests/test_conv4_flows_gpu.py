"""Image-shaped flows whose conditioners use 4 x 4 convolutions with padding="same" (one zero before the image, two after), on the
device under the knob ``conv_k4``, against the REAL reference's goldens (tests/golden/conv4/conv4_*.npz,
tests/golden/make_golden_conv4.py), with the bounds tests/test_conv5_flows_gpu.py holds the same quantities to: log_prob, the
layer loop's backward and forward at the fixtures' 4 rows, 100 rows through the recorded op list and the small-batch graph against
the fp64 CPU mirror; every 4 x 4 convolution counted on usf_conv2d_same_f32 / usf_conv2d_same_ctx_f32, in the backward on the
mirrored entry point (usf_conv2d_same_pad_f32), and none on F.conv2d; log_prob under autograd on the device training path (loss and
every gradient against the reference's fp64 run stored beside the fixtures, the weight gradients counted on
usf_conv_wgrad_k4_f32), Flow.fit eager and replayed against the reference's own 2-epoch SGD run, and
with SGD and Adam on the soft-trained flow against torch autograd; with the knob off the same flows on torch's convolution and autograd, as before."""
import glob
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from cond_image_cases import default_double, run_layers

DEV = "cuda:0"
pytestmark = pytest.mark.gpu
DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "conv4")
CASES = ["conv4_cond_c32", "conv4_cond_c64", "conv4_plain_c8"]


def load(name, device="cpu", dtype=torch.float32, override=None):
    """(mirror USFlow built as the generator builds the reference's, arrays); override: conditioner arguments to change (the
    arrays' reference results then no longer apply)"""
    from image_synth import synth_image_params_
    from usflows_amd import networks
    from usflows_amd.flows import USFlow
    z = np.load(os.path.join(DIR, name + ".npz"), allow_pickle=False)
    d = json.loads(str(z["spec"]))
    seed = d["seed"]
    dims = d["in_dims"]
    torch.manual_seed(d["seed"])
    base = torch.distributions.Laplace(torch.zeros(dims, dtype=dtype, device=device), torch.ones(dims, dtype=dtype, device=device))
    cond = d["cond_cls"] == "CondConvNet2D"
    flow = USFlow(base, dims, d["coupling_blocks"], getattr(networks, d["cond_cls"]), dict(d["cond_args"], **(override or {})),
                  householder=d["householder"], affine_conjugation=d["affine_conjugation"], **(dict(soft_training=True) if cond else {}))
    synth_image_params_(flow, d["seed"])
    if dtype == torch.float64:
        flow = flow.double()
        for l in flow.layers:
            if hasattr(l, "mask") and torch.is_tensor(l.mask):
                l.mask = l.mask.double()
    if device != "cpu":
        flow = flow.to(device)
    return flow, {k: torch.from_numpy(z[k]) for k in z.files if k != "spec"}, cond


class Counter:
    """counts the 4 x 4 convolutions on the device entry points (plain / ctx: torch's placement; mirror: the data gradient's) and
    on torch's convolution"""

    def __init__(self, monkeypatch):
        from usflows_amd import _ext
        self.plain = self.ctx = self.torch4 = self.mirror = 0
        real, real_ctx, real_f, real_pad = _ext.conv2d_same, _ext.conv2d_same_ctx, F.conv2d, _ext.conv2d_same_pad

        def pad(x, planes, cout, ks, pad_before, *a, **k):
            assert ks == 4 and pad_before == 2
            self.mirror += 1
            return real_pad(x, planes, cout, ks, pad_before, *a, **k)

        def plain(x, planes, cout, ks, *a, **k):
            self.plain += ks == 4
            return real(x, planes, cout, ks, *a, **k)

        def ctx(x, planes, cout, ks, *a, **k):
            self.ctx += ks == 4
            return real_ctx(x, planes, cout, ks, *a, **k)

        def fconv(inp, weight, *a, **k):
            self.torch4 += inp.is_cuda and tuple(weight.shape[2:]) == (4, 4)         # (the CPU mirror's reference runs do not count)
            return real_f(inp, weight, *a, **k)

        monkeypatch.setattr(_ext, "conv2d_same", plain)
        monkeypatch.setattr(_ext, "conv2d_same_ctx", ctx)
        monkeypatch.setattr(_ext, "conv2d_same_pad", pad)
        monkeypatch.setattr(F, "conv2d", fconv)


def _n_conv4(flow):
    return sum(1 for m in flow.modules() if isinstance(m, torch.nn.Conv2d) and m.kernel_size == (4, 4))


rel = lambda got, want: ((got.cpu().double() - want).abs().max() / want.abs().max()).item()   # noqa: E731


@pytest.mark.parametrize("name", CASES)
def test_conv4_flow_on_device_matches_reference(name, monkeypatch):
    from usflows_amd.config import config
    monkeypatch.setattr(config, "conv_k4", True)
    cnt = Counter(monkeypatch)
    flow, a, cond = load(name, device=DEV)
    n4 = _n_conv4(flow)
    assert n4 >= 8
    x, zin = a["x"].to(DEV), a["zin"].to(DEV)
    with torch.no_grad():
        if cond:
            ctx = a["ctx"].to(DEV)
            assert rel(flow.log_prob(x, ctx), a["log_prob64_ctx"]) <= 1e-5
            assert rel(flow.log_prob(x), a["log_prob64_noctx"]) <= 1e-5
            assert rel(run_layers(flow, x, ctx, True), a["backward64_ctx"]) <= 1e-5
            assert rel(run_layers(flow, zin, ctx, False), a["forward64_ctx"]) <= 1e-5
            passes = 4
        else:
            assert rel(flow.log_prob(x), a["log_prob64"]) <= 1e-5
            assert rel(flow.backward(x), a["backward64"]) <= 1e-5
            assert rel(flow._forward(zin), a["forward64"]) <= 1e-5
            passes = 3
        xs = flow.sample([5])
        assert xs.shape == (5, 16, 7, 7) and torch.isfinite(xs).all()
    n_cpl = sum(1 for l in flow.layers if type(l).__name__ == "MaskedCoupling")
    assert cnt.torch4 == 0 and cnt.mirror == 0, "a 4 x 4 convolution went to F.conv2d (or an inference pass to the mirrored placement)"
    assert cnt.plain + cnt.ctx >= passes * n4
    assert (cnt.ctx >= passes * n_cpl) if cond else cnt.ctx == 0


@pytest.mark.parametrize("name", CASES)
def test_conv4_flow_100_rows_through_the_op_list_and_the_graph(name, monkeypatch):
    from usflows_amd.config import config
    monkeypatch.setattr(config, "conv_k4", True)
    flow, a, cond = load(name, device=DEV)
    g = torch.Generator().manual_seed(9)
    x = torch.rand(100, 16, 7, 7, generator=g)
    ctx = 2.0 * torch.rand(100, 1, generator=g) if cond else None
    with default_double():
        f64, _, _ = load(name, dtype=torch.float64)
        with torch.no_grad():
            want = f64.log_prob(x.double(), ctx.double()) if cond else f64.log_prob(x.double())
    cnt = Counter(monkeypatch)
    xd, cd = x.to(DEV), (ctx.to(DEV) if cond else None)
    call = lambda: flow.log_prob(xd, cd) if cond else flow.log_prob(xd)   # noqa: E731
    key = (tuple(xd.shape), DEV) + (("ctx",) if cond else ())
    with torch.no_grad():
        flow.graph_max_rows, flow.list_max_rows = 0, 0
        eager = call()
        assert rel(eager, want) <= 1e-5
        flow.graph_max_rows, flow.list_max_rows = 256, 4096                    # the op list: recorded at the second sighting
        outs = [call() for _ in range(4)]
        plan = flow._loop_lists[key][1]
        assert plan is not None, "the pass of a 4 x 4 flow did not record as an op list"
        assert all(torch.equal(o, eager) for o in outs)
        flow.list_max_rows = 0                                                 # the small-batch graph
        outs = [call() for _ in range(3)]
        assert key in flow._loop_graphs and not getattr(flow, "_loop_graph_off", False)
        assert all(torch.equal(o, eager) for o in outs)
    assert cnt.torch4 == 0


@pytest.mark.parametrize("name", CASES)
def test_knob_off_runs_the_convolutions_on_torch(name, monkeypatch):
    """conv_k4 = 0: no 4 x 4 convolution reaches the device entry points, the results hold as before"""
    from usflows_amd.config import config
    monkeypatch.setattr(config, "conv_k4", False)
    cnt = Counter(monkeypatch)
    flow, a, cond = load(name, device=DEV)
    x = a["x"].to(DEV)
    with torch.no_grad():
        if cond:
            assert rel(flow.log_prob(x, a["ctx"].to(DEV)), a["log_prob64_ctx"]) <= 1e-5
        else:
            assert rel(flow.log_prob(x), a["log_prob64"]) <= 1e-5
    assert cnt.plain == 0 and cnt.ctx == 0 and cnt.mirror == 0 and cnt.torch4 >= _n_conv4(flow)


def _grads64(name, override=None):
    """(loss, {parameter: gradient}) of -mean(log_prob): the REFERENCE's fp64 run (tests/golden/conv4/<case>_grads*.npz); for a
    case with changed conditioner arguments, which the reference did not run, the fp64 CPU mirror's (modules bit-equal to the
    reference's, tests/test_conv4_cpu.py)"""
    if not override:
        g = {}
        for path in sorted(glob.glob(os.path.join(DIR, name + "_grads*.npz"))):
            with np.load(path, allow_pickle=False) as z:
                g.update({k[2:]: torch.from_numpy(z[k]) for k in z.files})
        assert len(g) >= 40, name
        with np.load(os.path.join(DIR, name + ".npz"), allow_pickle=False) as z:
            return float(z["loss64"]), g
    with default_double():
        f64, a, cond = load(name, dtype=torch.float64, override=override)
        x = a["x"].double()
        loss = -(f64.log_prob(x, a["ctx"].double()) if cond else f64.log_prob(x)).mean()
        loss.backward()
    return loss.item(), {k: p.grad.detach() for k, p in f64.named_parameters() if p.grad is not None}


def _train_once(name, monkeypatch, knob, override=None):
    from golden_util import grads_close
    from usflows_amd import _ext
    from usflows_amd.config import config
    monkeypatch.setattr(config, "conv_k4", knob)
    calls = []
    real = _ext.conv_wgrad_k4
    monkeypatch.setattr(_ext, "conv_wgrad_k4", lambda *a_, **k_: (calls.append(1), real(*a_, **k_))[1])
    cnt = Counter(monkeypatch)
    flow, a, cond = load(name, device=DEV, override=override)
    x = a["x"].to(DEV)
    conds = [l.conditioner for l in flow.layers if type(l).__name__ == "MaskedCoupling"]
    served = [c.train_on_device(x) for c in conds]
    flow.zero_grad(set_to_none=True)
    loss = -(flow.log_prob(x, a["ctx"].to(DEV)) if cond else flow.log_prob(x)).mean()
    loss.backward()
    loss64, g64 = _grads64(name, override)
    assert abs(loss.item() - loss64) <= 1e-5 * abs(loss64)
    grads_close(dict(flow.named_parameters()), g64)
    return served, len(calls), cnt, _n_conv4(flow)


@pytest.mark.parametrize("name", CASES)
def test_conv4_flow_trains_on_the_device(name, monkeypatch):
    """every fixture as it is: (b)'s 64-channel GatedConv runs its gate convolution in two halves, (c)'s 8 hidden channels take
    their kernel-1 weight gradients from the wide kernel -- both under the same knob"""
    served, n_wg, cnt, n4 = _train_once(name, monkeypatch, True)
    assert served and all(served), "train_on_device declined a 4 x 4 conditioner"
    assert n_wg == n4, "the 4 x 4 weight gradients did not all come from usf_conv_wgrad_k4_f32"
    assert cnt.torch4 == 0 and cnt.plain + cnt.ctx >= n4
    assert cnt.mirror == n4, "the 4 x 4 data gradients did not all run on the mirrored placement"


@pytest.mark.parametrize("name", CASES)
def test_knob_off_trains_under_torch_autograd(name, monkeypatch):
    served, n_wg, cnt, n4 = _train_once(name, monkeypatch, False)
    assert not any(served) and n_wg == 0 and cnt.plain == 0 and cnt.ctx == 0 and cnt.mirror == 0 and cnt.torch4 > 0


def test_knob_off_leaves_the_3x3_twins_of_b_and_c_declined(monkeypatch):
    """the two side routes belong to the knob: off, hidden widths 64 (gated) and 8 decline the device training path at
    kernel_size 3 as on the parent commit"""
    from usflows_amd.config import config
    monkeypatch.setattr(config, "conv_k4", False)
    monkeypatch.setattr(config, "conv_k5", False)
    for name in ("conv4_cond_c64", "conv4_plain_c8"):
        flow, a, _ = load(name, device=DEV, override=dict(kernel_size=3))
        x = a["x"].to(DEV)
        got = [l.conditioner.train_on_device(x) for l in flow.layers if type(l).__name__ == "MaskedCoupling"]
        assert got == [False] * len(got), (name, got)


def test_fit_eager_and_replayed_matches_the_reference_run(monkeypatch):
    """Flow.fit of the unconditional 4 x 4 flow at 16 hidden channels against the reference's own 2-epoch SGD run (96 rows from seed
    77, batch 32, shuffle under numpy seed 5; tests/golden/make_golden_conv4.py says why not the soft-trained (a): its noise comes
    from the generator of the device it runs on), eager and replayed, with the bounds of
    test_image_wide_training_gpu.py::test_fit_eager_and_replayed_matches_the_reference_run: losses 2e-4, parameters 2e-3 of the
    tensor's largest entry, every tensor's total update 1e-2 of the update's largest entry"""
    from usflows_amd import _ext
    from usflows_amd.config import config
    monkeypatch.setattr(config, "conv_k4", True)
    z = np.load(os.path.join(DIR, "conv4_fit_plain_c16.npz"), allow_pickle=False)
    spec = json.loads(str(z["spec"]))
    losses_ref, lr = [float(v) for v in z["losses"]], float(z["lr"])
    sd_ref = {k[3:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("sd/")}
    data = torch.rand(spec["rows"], *spec["in_dims"], generator=torch.Generator().manual_seed(spec["data_seed"]))
    steps = 2 * (data.shape[0] // 32)
    for graph in ("0", "1"):
        monkeypatch.setenv("USFLOWS_AMD_TRAIN_GRAPH", graph)
        flow, _, _ = load("conv4_fit_plain_c16", device=DEV)
        sd0 = {k: v.detach().cpu().double().clone() for k, v in flow.state_dict().items()}
        with monkeypatch.context() as m:
            wg = []
            real = _ext.conv_wgrad_k4
            m.setattr(_ext, "conv_wgrad_k4", lambda *a_, **k_: (wg.append(1), real(*a_, **k_))[1])
            cnt = Counter(m)
            ds = torch.utils.data.TensorDataset(data, torch.zeros(data.shape[0]))
            np.random.seed(spec["np_seed"])
            losses = flow.fit(ds, optim=torch.optim.SGD, optim_params=dict(lr=lr), batch_size=32, shuffle=True, device=torch.device(DEV),
                              epochs=2)
        assert len(wg) > 0 and cnt.torch4 == 0, "Flow.fit did not train the 4 x 4 convolutions on the device"
        replays = (flow.__dict__.get("_train_graph_state") or {}).get("replays", 0)
        assert (replays > 0) == (graph == "1"), (graph, replays, steps)
        sd = flow.state_dict()
        worst, worst_up, moved = (0.0, ""), (0.0, ""), 0
        for k, v in sd_ref.items():
            d = (sd[k].cpu().double() - v.double()).abs().max().item()
            worst = max(worst, (d / max(v.abs().max().item(), 1e-3), k))
            up = (v.double() - sd0[k]).abs().max().item()
            if up > 0:
                moved += 1
                worst_up = max(worst_up, (d / up, k))
        print(f"graph {graph}: losses {[float(l) for l in losses]} (reference {losses_ref}); replays {replays} of {steps}; "
              f"worst parameter {worst}; worst update {worst_up}")
        for l, r in zip(losses, losses_ref):
            assert abs(float(l) - r) < 2e-4 * abs(r), (graph, losses, losses_ref)
        assert worst[0] < 2e-3, (graph, worst)
        assert moved >= 30 and worst_up[0] < 1e-2, (graph, worst_up)


def test_fit_of_the_soft_trained_flow_matches_torch_autograd(monkeypatch):
    """6 steps of Flow.fit at batch 32 of the soft-trained CondConvNet2D flow (a), with SGD and with Adam: the device training
    path, eager and captured / replayed, against torch autograd on the same GPU (image_train off) from the same seed -- every
    parameter within 2 % of what the steps changed (the bound of the conditional 3 x 3 flows' fit test)"""
    from usflows_amd import _ext
    from usflows_amd.config import config
    monkeypatch.setattr(config, "conv_k4", True)
    data = torch.rand(192, 16, 7, 7, generator=torch.Generator().manual_seed(3))
    ds = torch.utils.data.TensorDataset(data, torch.zeros(data.shape[0]))
    for optim, params in ((torch.optim.SGD, dict(lr=1e-3)), (torch.optim.Adam, dict(lr=1e-4))):
        runs = {}
        for mode in ("replayed", "eager", "autograd"):
            monkeypatch.setattr(config, "image_train", mode != "autograd")
            monkeypatch.setenv("USFLOWS_AMD_TRAIN_GRAPH", "1" if mode == "replayed" else "0")
            flow, _, _ = load("conv4_cond_c32", device=DEV)
            init = {k: v.detach().cpu().double().clone() for k, v in flow.state_dict().items()}
            wg = []
            real = _ext.conv_wgrad_k4
            monkeypatch.setattr(_ext, "conv_wgrad_k4", lambda *a_, **k_: (wg.append(1), real(*a_, **k_))[1])
            torch.manual_seed(0)
            flow.fit(ds, optim=optim, optim_params=dict(params), batch_size=32, shuffle=False, device=torch.device(DEV), epochs=1)
            monkeypatch.setattr(_ext, "conv_wgrad_k4", real)
            st = flow.__dict__.get("_train_graph_state") or {}
            runs[mode] = ({k: v.detach().cpu().double() for k, v in flow.state_dict().items()}, len(wg), st.get("replays", 0))
        assert runs["replayed"][1] > 0 and runs["eager"][1] > 0 and runs["autograd"][1] == 0
        assert runs["replayed"][2] > 0 and runs["eager"][2] == 0, "the step was not captured and replayed"
        sd_ref = runs["autograd"][0]
        for mode in ("replayed", "eager"):
            moved = 0
            for k, v in sd_ref.items():
                change = (v - init[k]).abs().max().item()
                if change == 0.0:
                    continue
                moved += 1
                d = (runs[mode][0][k] - v).abs().max().item()
                assert d <= 2e-2 * change, (optim.__name__, mode, k, d, change)
            assert moved >= 20
