#!/usr/bin/env python3
"""Inference of image flows whose feature maps have more than 256 pixels -- the reference's datasets without space-to-depth,
MNIST [1, 28, 28] and CIFAR [3, 32, 32] -- with the knob ``conv_band`` on (the row-banded kernel usf_conv2d_same_band_f32) against
a parent checkout (torch's convolution there), and the untouched [16, 7, 7] model on both as the control.

One run measures ONE checkout under ONE value of the knob and appends its entries to the JSON file (the method of
tools/bench_conv5.py); this commit and a parent checkout alternate on one MI355X, two runs each:

    python3 tools/bench_conv_band.py --root <parent checkout> --label parent --out profiles/conv_band_bench.json   (a checkout without the knob)
    python3 tools/bench_conv_band.py --knob 1 --label on --out profiles/conv_band_bench.json                       (and again, both)

  logprob100/<flow>    log_prob of the 100 rows the reference evaluates in (the replayed small-batch form): ms, median of the timed calls
  logprob8192/<flow>   log_prob of 8192 rows: ms
  sample100/<flow>     sample([100], seed): ms
  groups/<flow>        (this commit only) B * bands of the 32 -> 32 layers' launches at 100 rows, from usf_conv2d_same_band_variant: with
                       fewer groups than compute units a launch leaves the rest idle
Flows: mnist = [1, 28, 28], cifar = [3, 32, 32], control = [16, 7, 7]; each 5 blocks, ConvNet2D(c_hidden 32, 3 gated layers, layer
norm, kernel 3), radial LogNormal base, prior_scale 1.0.  Prints the summary: per label and workload the median over the runs and
the spread between the runs of one label."""
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
ap.add_argument("--knob", type=int, default=1, help="conv_band (ignored by a checkout that has no such knob)")
ap.add_argument("--only", nargs="+", default=None)
ap.add_argument("--timeout", type=int, default=200, help="seconds per child process")
ap.add_argument("--out", default=None)
ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
args = ap.parse_args()

FLOWS = {"mnist": [1, 28, 28], "cifar": [3, 32, 32], "control": [16, 7, 7]}
WORK = [f"{k}/{f}" for f in ("mnist", "cifar") for k in ("logprob100", "logprob8192", "sample100")] + \
    ["logprob100/control", "logprob8192/control"]


def timed(fn, warm, n):
    import torch
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts)


def child(work):
    sys.path.insert(0, args.root)
    import warnings
    import torch
    from usflows_amd import _ext
    from usflows_amd import distributions as UD
    from usflows_amd.config import config
    from usflows_amd.flows import USFlow
    from usflows_amd.networks import ConvNet2D
    warnings.simplefilter("ignore")
    has_knob = "conv_band" in config._KNOBS
    if has_knob:
        config.conv_band = bool(args.knob)
    dev = "cuda:0"
    kind, which = work.split("/", 1)
    dims = FLOWS[which]
    torch.manual_seed(0)
    base = UD.RadialDistribution(device="cpu", p=1.0, loc=torch.zeros(dims),
                                 norm_distribution=UD.LogNormal(loc=torch.ones([1]) * 6, scale=torch.ones([1]) * .35, device="cpu"))
    cond = dict(c_in=dims[0], c_hidden=32, num_layers=3, padding="same", kernel_size=3, normalize_layers=True, gating=True)
    flow = USFlow(base, dims, 5, ConvNet2D, cond, prior_scale=1.0, lu_transform=1, householder=0, affine_conjugation=True).to(dev)
    out = {}
    with torch.no_grad():
        if kind == "sample100":
            out["ms"] = timed(lambda: flow.sample([100], seed=7), 6, 50)
        else:
            rows = int(kind[len("logprob"):])
            x = torch.rand(rows, *dims, device=dev)
            out["ms"] = timed(lambda: flow.log_prob(x), 6, 10 if rows > 1000 else 100)
    if has_knob and args.knob and kind == "logprob100" and dims[1] * dims[2] > 256:
        a = _ext.conv2d_same_band_variant(100, 32, 32, dims[1], dims[2], 3)
        out["groups"] = a["groups"]
    print("RESULT " + json.dumps(out))


if args.child:
    child(args.child)
    sys.exit(0)

entries = {}
for w in WORK:
    if args.only and w not in args.only:
        continue
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--root", args.root, "--knob", str(args.knob), "--child", w],
                       capture_output=True, text=True, timeout=args.timeout)
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
    if r.returncode != 0 or not line:
        sys.exit(f"{w}: child failed ({r.returncode}): {r.stderr[-800:]}")
    for k, v in json.loads(line[-1][7:]).items():
        key = w if k == "ms" else f"{k}/{w.split('/', 1)[1]}"
        entries[key] = v
        print(f"{args.label:8s} {key:36s} {v:9.3f}", flush=True)

if args.out:
    doc = json.load(open(args.out)) if os.path.exists(args.out) else {"runs": {}, "summary": {}}
    doc["runs"].setdefault(args.label, []).append(entries)
    doc["summary"] = {}
    for label, runs in doc["runs"].items():
        for w in sorted({k for r in runs for k in r}):
            vals = [r[w] for r in runs if w in r]
            doc["summary"].setdefault(w, {})[label] = dict(median=statistics.median(vals), spread=max(vals) - min(vals), runs=len(vals))
    with open(args.out, "w") as fh:
        json.dump(doc, fh, indent=1, sort_keys=True)
    for w, by in sorted(doc["summary"].items()):
        print(w, {k: (round(v["median"], 3), round(v["spread"], 3)) for k, v in by.items()})
