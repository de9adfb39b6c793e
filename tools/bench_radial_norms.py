#!/usr/bin/env python3
"""The live MNIST flow (bench.py's mnist_live: [16,7,7], 15 blocks, 3 gated layers, prior_scale 1.0) over a radial base whose
radius distribution is a ``WeibullMM`` x 20 (p = 1) -- served by the radial kernels from this commit on, the distribution
object's op chain before -- and over the ``LogNormal(6, .35)`` of the live configuration as the check of the untouched kinds.

One run measures ONE checkout and appends its entries to the JSON file; the comparison is made by running this same file
against a parent checkout on the same box, the two alternating, two runs each:

    python3 tools/bench_radial_norms.py --label this --out profiles/radial_norms_bench.json
    python3 tools/bench_radial_norms.py --root <parent checkout> --label parent --out profiles/radial_norms_bench.json    (and again)

  fit/<base>        Flow.fit with SophiaG at batch 32 on resident rows: ms per step over whole epochs after a warm-up fit, and
                    how many of the last fit's steps were replays of the captured step
  log_prob/<base>   Flow.log_prob at 65 536 rows under no_grad: ms per call, median of the timed calls

The file then holds, per label and workload, the median over the runs and the spread between the runs of one label: a
difference between the labels means something where it exceeds that spread.  Prints the summary."""
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
ap.add_argument("--bases", nargs="+", default=["weibullmm", "lognormal"])
ap.add_argument("--steps", type=int, default=60)
ap.add_argument("--rows", type=int, default=65536)
ap.add_argument("--timeout", type=int, default=300, help="seconds per child process")
ap.add_argument("--out", default=None)
ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
args = ap.parse_args()


def child(base_kind):
    """both figures of one base, in the checkout --root"""
    sys.path.insert(0, args.root)
    import warnings
    import numpy as np
    import torch
    import bench
    from usflows_amd import distributions as UD
    from usflows_amd.flows import USFlow
    from usflows_amd.networks import ConvNet2D
    from usflows_amd.sophia import SophiaG
    cfg = bench.IMAGE_CONFIGS["mnist_live"]
    dims = list(cfg["in_dims"])
    torch.manual_seed(0)
    if base_kind == "lognormal":
        nd = UD.LogNormal(loc=torch.ones([1]) * 6, scale=torch.ones([1]) * .35, device="cpu")
    else:
        # (MixtureModel stores the scales through log(exp(x) - 1), which overflows in fp32 beyond 88)
        nd = UD.WeibullMM(scale=20 + 60 * torch.rand([20]), concentration=1 + torch.rand([20]), mixture_weights=torch.ones([20]) / 20,
                          device="cpu")
    base = UD.RadialDistribution(device="cpu", p=float("1"), loc=torch.zeros(dims), norm_distribution=nd)
    flow = USFlow(base, dims, cfg["blocks"], ConvNet2D, dict(cfg["cond"]), prior_scale=cfg["prior_scale"],
                  householder=cfg["householder"], affine_conjugation=True)
    bench._condition_image_flow(flow, seed=0)
    flow = flow.to("cuda:0")
    n = 32 * args.steps
    data = torch.rand(n, *dims, generator=torch.Generator().manual_seed(1))
    ds = torch.utils.data.TensorDataset(data, torch.zeros(n))

    def fit():
        np.random.seed(5)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        flow.fit(ds, optim=SophiaG, optim_params=dict(lr=1e-6), batch_size=32, shuffle=False, device=torch.device("cuda:0"), epochs=1)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / args.steps * 1e3

    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        fit()                                        # allocations, plans, the first capture
        ms = [fit() for _ in range(3)]
    st = flow.__dict__.get("_train_graph_state") or {}
    out = dict(fit=dict(ms=round(statistics.median(ms), 4), fit_replays=st.get("replays", 0), of_steps=args.steps,
                        warnings=sorted({str(w.message)[:120] for w in caught})))
    x = torch.rand(args.rows, *dims, generator=torch.Generator().manual_seed(2)).to("cuda:0")
    ts = []
    with torch.no_grad():
        for i in range(8):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            lp = flow.log_prob(x)
            torch.cuda.synchronize()
            if i >= 3:
                ts.append((time.perf_counter() - t0) * 1e3)
    assert bool(torch.isfinite(lp).all()), "log_prob is not finite on the benchmark rows"
    out["log_prob"] = dict(ms=round(statistics.median(ts), 4), rows=args.rows)
    print(json.dumps(out))


def measure(base_kind):
    cmd = [sys.executable, os.path.abspath(__file__), "--root", args.root, "--steps", str(args.steps), "--rows", str(args.rows),
           "--child", base_kind]
    r = subprocess.run(cmd, cwd=args.root, capture_output=True, text=True, timeout=args.timeout)
    if r.returncode != 0:
        raise RuntimeError(f"the measurement of {base_kind} failed (rc {r.returncode}): {r.stderr[-800:]}")
    return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])


def main():
    if args.child:
        return child(args.child)
    entries = []
    for b in args.bases:
        m = measure(b)
        entries.append(dict(label=args.label, workload=f"fit/{b}", **m["fit"]))
        entries.append(dict(label=args.label, workload=f"log_prob/{b}", **m["log_prob"]))
    out = dict(what="mnist_live-shaped flow over a radial base: Flow.fit ms per step at batch 32 (and replays among the last fit's "
                    "steps), log_prob ms per call at 65 536 rows", runs=[])
    if args.out and os.path.exists(args.out):
        out = json.load(open(args.out))
    out["runs"].extend(entries)
    groups = {}
    for e in out["runs"]:
        groups.setdefault(f"{e['label']}/{e['workload']}", []).append(e)
    out["summary"] = {k: dict(median_ms=round(statistics.median(e["ms"] for e in v), 4), runs=len(v),
                              spread=round((max(e["ms"] for e in v) - min(e["ms"] for e in v)) / statistics.median(e["ms"] for e in v), 4),
                              **({"fit_replays": [e["fit_replays"] for e in v], "of_steps": v[0]["of_steps"]} if "fit_replays" in v[0] else {}))
                      for k, v in groups.items()}
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(json.dumps(out, indent=1) + "\n")
    print(json.dumps(out["summary"]))


if __name__ == "__main__":
    main()
