#!/usr/bin/env python3
"""Conditional image flows against their unconditional counterpart (the MNIST-shaped model of the reference's image
configurations): log_prob ms at 65 536 and 100 rows and Flow.fit ms per step at batch 32 (SGD, 3 epochs of 8 batches, the
first epoch not counted) for  uncond = ConvNet2D,  soft = ConvNet2D with soft_training,  cond = CondConvNet2D with
soft_training (log_prob with a per-row context).  Prints one JSON line.   python3 tools/bench_cond_image.py"""
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from image_synth import synth_image_params_  # noqa: E402
from usflows_amd.flows import USFlow  # noqa: E402
from usflows_amd.networks import CondConvNet2D, ConvNet2D  # noqa: E402

DEV = torch.device("cuda:0")
DIMS = [16, 7, 7]
COND = dict(c_in=16, c_hidden=32, num_layers=3, padding="same", kernel_size=3, normalize_layers=True, gating=True)


def make(cls, soft):
    torch.manual_seed(11)
    flow = USFlow(torch.distributions.Laplace(torch.zeros(DIMS, device=DEV), torch.ones(DIMS, device=DEV)), DIMS, 2, cls,
                  dict(COND), householder=1, affine_conjugation=True, soft_training=soft)
    synth_image_params_(flow, 11)
    return flow.to(DEV)


def time_log_prob(flow, B, ctx, n):
    x = torch.rand(B, *DIMS, device=DEV)
    c = (2.0 * torch.rand(B, 1, device=DEV)) if ctx else None
    with torch.no_grad():
        for _ in range(4):
            flow.log_prob(x, c)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            flow.log_prob(x, c)
        torch.cuda.synchronize()
    return (time.perf_counter() - t0) / n * 1e3


def time_fit(flow, batch=32, steps_per_epoch=8):
    data = torch.rand(batch * steps_per_epoch, *DIMS)
    ds = torch.utils.data.TensorDataset(data, torch.zeros(data.shape[0]))
    flow.fit(ds, optim=torch.optim.SGD, optim_params=dict(lr=1e-4), batch_size=batch, shuffle=False, device=DEV, epochs=1)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    flow.fit(ds, optim=torch.optim.SGD, optim_params=dict(lr=1e-4), batch_size=batch, shuffle=False, device=DEV, epochs=2)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / (2 * steps_per_epoch) * 1e3


def main():
    out = {}
    for key, cls, soft, ctx in (("uncond", ConvNet2D, False, False), ("soft", ConvNet2D, True, False),
                                ("cond", CondConvNet2D, True, True)):
        flow = make(cls, soft)
        out[key] = dict(log_prob_65536_ms=round(time_log_prob(flow, 65536, ctx, 20), 4),
                        log_prob_100_ms=round(time_log_prob(flow, 100, ctx, 200), 4),
                        fit_step_b32_ms=round(time_fit(flow), 4))
    out["ratio_cond_vs_uncond_log_prob_65536"] = round(out["cond"]["log_prob_65536_ms"] / out["uncond"]["log_prob_65536_ms"], 4)
    out["ratio_soft_vs_uncond_fit_step"] = round(out["soft"]["fit_step_b32_ms"] / out["uncond"]["fit_step_b32_ms"], 4)
    out["ratio_cond_vs_uncond_fit_step"] = round(out["cond"]["fit_step_b32_ms"] / out["uncond"]["fit_step_b32_ms"], 4)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
