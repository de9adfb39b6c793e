"""Flow.fit with torch.optim.Adam(lr=1e-3, weight_decay=0.1) against the REAL reference's own run of the same six steps
(tests/golden/make_golden_fit_adam.py: fp32 and fp64, the second case with gradient_clip=1.0) -- on the CPU through the
mirror and on the MI355X through usf_adam_step_f32 and the clip kernels.

Bound, per tensor and for the losses: distance to the reference's fp64 run <= 4 x the reference's own fp32-fp64 distance
+ the floor of the SGD fit goldens (tests/test_modules_cpu.py / tests/test_training_gpu.py: 2e-5 on the CPU, 5e-5 on the
device, of max(1, largest entry); losses 1e-4 relative).  The factor 4 allows for the device gradients' bf16x3 rounding on
top of fp32.  The measured ratios are printed (run with -s) and recorded in profiles/fit_optim_parity.md."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from golden_util import load_case  # noqa: E402
from model_util import build_flow  # noqa: E402

CASES = ["synth_d7_k3_hh0_laplace", "synth_d16_k3_hh1_radial2"]


def _load(name):
    z = np.load(os.path.join(HERE, "golden", "fitadam", "fitadam_" + name + ".npz"), allow_pickle=False)
    sd32 = {k[5:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("sd32/")}
    sd64 = {k[5:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("sd64/")}
    clip = float(z["gradient_clip"])
    return (torch.from_numpy(z["data"]), [float(v) for v in z["losses32"]], [float(v) for v in z["losses64"]], sd32, sd64,
            None if clip < 0 else clip)


def _run_and_check(name, device, floor):
    spec, sd, _ = load_case(name)
    data, l32, l64, sd32, sd64, clip = _load(name)
    flow = build_flow(spec, sd, device=device) if device != "cpu" else build_flow(spec, sd)
    ds = torch.utils.data.TensorDataset(data, torch.zeros(data.shape[0]))
    np.random.seed(5)
    losses = flow.fit(ds, optim=torch.optim.Adam, optim_params=dict(lr=1e-3, weight_decay=0.1), batch_size=32, shuffle=True,
                      gradient_clip=clip, device=torch.device(device), epochs=2)
    bad = []
    for got, a, b in zip(losses, l32, l64):
        own, d = abs(a - b), abs(float(got) - b)
        print(f"{name} [{device}] loss: distance to fp64 {d:.3e}, reference fp32-fp64 {own:.3e}")
        if d > 4 * own + 1e-4 * abs(b):
            bad.append(("loss", d, own))
    got_sd, n = flow.state_dict(), 0
    for k, ref in sd64.items():
        if not ref.is_floating_point() or k not in got_sd:
            continue
        n += 1
        d = (got_sd[k].detach().cpu().double().reshape(ref.shape) - ref).abs()
        own = (sd32[k].double() - ref).abs().max().item()
        bound = 4 * own + floor * max(1.0, ref.abs().max().item())
        print(f"{name} [{device}] {k}: distance to fp64 {d.max().item():.3e}, reference fp32-fp64 {own:.3e}, "
              f"ratio {d.max().item() / max(own, 1e-30):.2f}")
        if d.max().item() > bound:
            bad.append((k, d.max().item(), own, torch.nonzero(d > bound).flatten().tolist()[:8]))
    assert n >= 20
    assert not bad, bad
    return flow


@pytest.mark.parametrize("name", CASES)
def test_mirror_fit_with_adam_reproduces_the_reference_run_cpu(name):
    _run_and_check(name, "cpu", 2e-5)


@pytest.mark.gpu
@pytest.mark.parametrize("name", CASES)
def test_device_fit_with_adam_reproduces_the_reference_run(name):
    flow = _run_and_check(name, "cuda:0", 5e-5)
    st = flow.__dict__.get("_train_graph_state")
    assert st is not None and st["replays"] > 0 and not getattr(flow, "_train_graph_failed", False)
