#!/usr/bin/env python3
"""Flow.fit's step at the reference's training batch of 32 with torch.optim.Adam, and with SophiaG under gradient_clip=1.0:
the step replayed as a hipGraph (this commit: usflows_amd/optim.py) against the eager step (the parent commit).

One run measures ONE checkout and appends its entries to the JSON file; the comparison is made by running this same file
against a parent checkout on the same box, the two alternating, two runs each:

    python3 tools/bench_fit_optim.py --label this --out profiles/fit_optim_bench.json
    python3 tools/bench_fit_optim.py --root <parent checkout> --label parent --out profiles/fit_optim_bench.json     (and again)

  adam/<config>      ``bench.py --mode fit --optim adam --batch 32 --config <config>`` of the checkout, run as a child process
                     for cfg2, gm_live and mnist_live: ms per step and how many of the timed steps were graph replays
  clip/gm_live       Flow.fit(gradient_clip=1.0) with SophiaG on the gm_live-shaped flow, timed here (bench.py has no clip):
                     ms per step over whole epochs of batch 32 after a warm-up fit, and the replays of the last fit

The file then holds, per label and workload, the median over the runs and the spread between the runs of one label --
the claim "not slower than the parent's eager step" holds where the difference exceeds that spread.  Prints the summary."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))), help="the checkout to measure")
ap.add_argument("--label", default="this")
ap.add_argument("--configs", nargs="+", default=["cfg2", "gm_live", "mnist_live"])
ap.add_argument("--steps", type=int, default=60)
ap.add_argument("--warmup", type=int, default=8)
ap.add_argument("--timeout", type=int, default=240, help="seconds per child process")
ap.add_argument("--out", default=None)
ap.add_argument("--clip-child", action="store_true", help=argparse.SUPPRESS)
args = ap.parse_args()


def bench_adam(config):
    # (the image configurations call their Flow.fit step --mode train; the flat ones --mode fit)
    mode = "train" if config.startswith(("mnist", "cifar")) else "fit"
    cmd = [sys.executable, os.path.join(args.root, "bench.py"), "--gpus", "1", "--mode", mode, "--optim", "adam", "--batch", "32",
           "--config", config, "--steps", str(args.steps), "--warmup", str(args.warmup), "--no-cpu-baseline", "--no-kernel-timing",
           "--no-fast-mode", "--no-also"]
    r = subprocess.run(cmd, cwd=args.root, capture_output=True, text=True, timeout=args.timeout)
    if r.returncode != 0:
        raise RuntimeError(f"bench.py failed for {config} (rc {r.returncode}): {r.stderr[-800:]}")
    o = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    ts = o.get("train_step") or {}
    return dict(ms_per_step=o["ms_per_step"], fit_replays=ts.get("graph_replays"), of_steps=ts.get("of_steps", o.get("steps")))


def clip_child():
    """Flow.fit(gradient_clip=1.0), SophiaG, the gm_live-shaped flow (10-D, 10 blocks, DenseNN [32, 32]) -- in the checkout"""
    sys.path.insert(0, args.root)
    import numpy as np
    import torch
    from oracle import usflows_oracle as orc
    from usflows_amd.synth import build_usflow
    from usflows_amd.sophia import SophiaG
    spec = orc.FlowSpec(10, 10, [32, 32], householder=0, affine_conjugation=True, conditioner="DenseNN", negative_slope=0.0)
    flow = build_usflow(spec, orc.synth_state_dict(spec, seed=3), device="cuda:0")
    rows = 32 * args.steps
    data = torch.rand(rows, 10, generator=torch.Generator().manual_seed(1))
    ds = torch.utils.data.TensorDataset(data, torch.zeros(rows))

    def fit():
        np.random.seed(5)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        flow.fit(ds, optim=SophiaG, optim_params=dict(lr=1e-6), batch_size=32, shuffle=False, gradient_clip=1.0,
                 device=torch.device("cuda:0"), epochs=1)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / args.steps * 1e3

    fit()                                        # allocations, plans, the first capture
    ms = [fit() for _ in range(3)]
    st = flow.__dict__.get("_train_graph_state") or {}
    print(json.dumps(dict(ms_per_step=round(statistics.median(ms), 4), fit_replays=st.get("replays", 0), of_steps=args.steps)))


def bench_clip():
    cmd = [sys.executable, os.path.abspath(__file__), "--root", args.root, "--steps", str(args.steps), "--clip-child"]
    r = subprocess.run(cmd, cwd=args.root, capture_output=True, text=True, timeout=args.timeout)
    if r.returncode != 0:
        raise RuntimeError(f"the clip measurement failed (rc {r.returncode}): {r.stderr[-800:]}")
    return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])


def main():
    if args.clip_child:
        return clip_child()
    entries = [dict(label=args.label, workload=f"adam/{c}", **bench_adam(c)) for c in args.configs]
    entries.append(dict(label=args.label, workload="clip/gm_live", **bench_clip()))
    out = dict(what="Flow.fit step at batch 32: ms per step and graph replays among the timed steps", runs=[])
    if args.out and os.path.exists(args.out):
        out = json.load(open(args.out))
    out["runs"].extend(entries)
    groups = {}
    for e in out["runs"]:
        groups.setdefault(f"{e['label']}/{e['workload']}", []).append(e)
    out["summary"] = {k: dict(median_ms=round(statistics.median(e["ms_per_step"] for e in v), 4), runs=len(v),
                              spread=round((max(e["ms_per_step"] for e in v) - min(e["ms_per_step"] for e in v))
                                           / statistics.median(e["ms_per_step"] for e in v), 4),
                              fit_replays=[e["fit_replays"] for e in v], of_steps=v[0]["of_steps"]) for k, v in groups.items()}
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(json.dumps(out, indent=1) + "\n")
    print(json.dumps(out["summary"]))


if __name__ == "__main__":
    main()
