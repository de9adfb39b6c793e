#!/usr/bin/env python3
"""A context on the planes pipeline against the paths that served it before, on the BASELINE cfg2 model (D = 784, 32 coupling
blocks, hidden [256, 256]) at 65 536 rows -- same process, the variants alternating round by round, HIP-event timed after warm-up:
  a  log_prob(x, ctx) on the planes plan                      c  log_prob(x) on the planes plan
  b  log_prob(x, ctx) with eng.use_planes = False (the fp32-activation plan)
  d  one training step (log_prob(x, ctx), backward of -mean) on the planes training path
  e  the same step with use_train_planes off (USFLOWS_AMD_TRAIN_PLANES=0: the fp32-row path)
Writes profiles/ctx_planes_bench.json and prints it as one JSON line.   python3 tools/bench_ctx_planes.py [--rows N] [--rounds R]"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from golden_util import load_case  # noqa: E402
from usflows_amd import _ext  # noqa: E402
from usflows_amd.synth import build_usflow  # noqa: E402

DEV = torch.device("cuda:0")


def timed(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=65536)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--train-iters", type=int, default=4)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ctx_planes_bench.json"))
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_ctx_planes.py measures on the GPU"
    spec, sd, _a = load_case("synth_d784_k32_cfg2")
    B = args.rows
    g = torch.Generator().manual_seed(1)
    x = torch.rand(B, spec.dim, generator=g).to(DEV)
    ctx = (2.0 * torch.rand(B, 1, generator=g)).to(DEV)

    infer = build_usflow(spec, sd, device="cuda:0")
    eng = infer.engine()

    def log_prob(planes, c):
        def run():
            eng.use_planes, eng.ctx_planes_min_rows = planes, 0     # (a): automatic mode with the context plans switched on
            with torch.no_grad():
                return infer.log_prob(x, c)
        return run

    def has_ctx_launch(p):
        return any(_ext.is_ctx_prefix(p["arr"][j]) for j in range(p["n"]))

    variants = dict(a=log_prob(None, ctx), b=log_prob(False, ctx), c=log_prob(None, None))
    outs = {k: f().clone() for k, f in variants.items()}
    torch.cuda.synchronize()
    assert any(p.get("planes") and p.get("has_ctx") and has_ctx_launch(p) for p in eng._plans.values()), "(a) did not take the planes plan"
    agree = ((outs["a"] - outs["b"]).abs() / outs["b"].abs()).max().item()

    train = {}
    for key, on in (("d", True), ("e", False)):
        flow = build_usflow(spec, sd, device="cuda:0")
        flow.engine().use_train_planes, flow.engine().train_ctx_planes_min_rows = on, 0

        def step(flow=flow):
            for p in flow.parameters():
                p.grad = None
            (-flow.log_prob(x, ctx).mean()).backward()
        train[key] = (flow, step)
    for key, (flow, step) in train.items():
        for _ in range(3):
            step()
        torch.cuda.synchronize()
        plan = flow.engine()._plan("backward", B, DEV, True, "nat", train=True)
        assert bool(plan.get("planes_train")) == (key == "d"), key
    for f in variants.values():
        for _ in range(3):
            f()
    torch.cuda.synchronize()

    ms = {k: [] for k in "abcde"}
    for _ in range(args.rounds):
        for k, f in variants.items():
            ms[k].append(timed(f, args.iters))
        for k, (_flow, step) in train.items():
            ms[k].append(timed(step, args.train_iters))
    med = {k: statistics.median(v) for k, v in ms.items()}
    out = dict(model="synth_d784_k32_cfg2", rows=B, rounds=args.rounds, iters=args.iters, train_iters=args.train_iters,
               ms={k: round(v, 4) for k, v in med.items()}, ms_rounds={k: [round(t, 4) for t in v] for k, v in ms.items()},
               a_over_b=round(med["a"] / med["b"], 4), d_over_e=round(med["d"] / med["e"], 4), a_over_c=round(med["a"] / med["c"], 4),
               log_prob_a_vs_b_max_rel=agree,
               what=dict(a="log_prob(x, ctx), planes plan", b="log_prob(x, ctx), fp32-activation plan", c="log_prob(x), planes plan",
                         d="training step with ctx, planes training path", e="training step with ctx, fp32-row path"))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(json.dumps(out) + "\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
