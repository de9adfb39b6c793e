#!/usr/bin/env python3
"""Training steps of an image flow whose feature maps have more than 64 pixels: a [4, 14, 14] flow (the reference's
experiments/mnist/mnist_usflow_gpu.yaml at space-to-depth 2 with a servable width: 5 coupling blocks, ConvNet2D with c_hidden 16,
4 gated layers, layer norm, Householder 1, conjugation) -- its weight gradients come from usf_conv_wgrad_wide_f32 from this
commit on, from torch autograd + MIOpen before -- and the untouched [16, 7, 7] MNIST model as the regression check.

One run measures ONE checkout and appends its entries to the JSON file; the comparison is made by running this same file
against a parent checkout on the same box, the two alternating, two or three runs each (the method of tools/bench_radial_norms.py):

    python3 tools/bench_image_wide.py --label this --out profiles/image_wide_bench.json
    python3 tools/bench_image_wide.py --root <parent checkout> --label parent --out profiles/image_wide_bench.json    (and again)

  fit32/<flow>      Flow.fit with Adam at batch 32 on resident rows (the replayed step): ms per step
  fit1024/wide      the same at the configuration file's batch of 1024
  step4096/wide     one training step (log_prob, backward) at 4096 rows: ms, median of the timed steps

--only fit32/mnist --steps 400 repeats the regression check with the per-fit capture diluted (every fit call runs three eager
steps and captures anew; at 40 steps they are a sixth of the timed time and most of its spread).

The file then holds, per label and workload, all runs, their median and the spread between them: a difference between the
labels means something where it exceeds the larger of the two spreads.  Prints the summary."""
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
ap.add_argument("--steps", type=int, default=40)
ap.add_argument("--only", nargs="+", default=None, help="workloads to run (default: all), e.g. fit32/mnist")
ap.add_argument("--timeout", type=int, default=240, help="seconds per child process")
ap.add_argument("--out", default=None)
ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
args = ap.parse_args()

FLOWS = {
    "wide": dict(dims=[4, 14, 14], blocks=5, cond=dict(c_in=4, c_hidden=16, num_layers=4, padding="same", kernel_size=3,
                                                      normalize_layers=True, gating=True)),
    "mnist": dict(dims=[16, 7, 7], blocks=2, cond=dict(c_in=16, c_hidden=32, num_layers=1, padding="same", kernel_size=3,
                                                      normalize_layers=True, gating=True)),
}
WORK = [("fit32", "wide"), ("fit1024", "wide"), ("step4096", "wide"), ("fit32", "mnist")]


def child(work):
    kind, which = work.split("/")
    sys.path.insert(0, args.root)
    import warnings
    import torch
    from usflows_amd.flows import USFlow
    from usflows_amd.networks import ConvNet2D
    warnings.simplefilter("ignore")
    f = FLOWS[which]
    dims, dev = f["dims"], "cuda:0"
    torch.manual_seed(0)
    flow = USFlow(torch.distributions.Laplace(torch.zeros(dims, device=dev), torch.ones(dims, device=dev)), dims, f["blocks"], ConvNet2D,
                  dict(f["cond"]), householder=1, affine_conjugation=True).to(dev)
    out = {}
    if kind.startswith("fit"):
        batch = int(kind[3:])
        n = batch * args.steps
        data = torch.rand(n, *dims, generator=torch.Generator().manual_seed(1))
        ds = torch.utils.data.TensorDataset(data, torch.zeros(n))
        kw = dict(optim=torch.optim.Adam, optim_params=dict(lr=1e-5), batch_size=batch, shuffle=False, device=torch.device(dev))
        flow.fit(ds, epochs=1, **kw)                               # warm-up: plans, capture
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        flow.fit(ds, epochs=2, **kw)
        torch.cuda.synchronize()
        out["ms"] = (time.perf_counter() - t0) * 1e3 / (2 * args.steps)
    else:
        rows = int(kind[4:])
        x = torch.rand(rows, *dims, device=dev)
        ts = []
        for i in range(3 + 9):
            for p in flow.parameters():
                p.grad = None
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            (-flow.log_prob(x).mean()).backward()
            torch.cuda.synchronize()
            if i >= 3:
                ts.append((time.perf_counter() - t0) * 1e3)
        out["ms"] = statistics.median(ts)
    print("RESULT " + json.dumps(out))


if args.child:
    child(args.child)
    sys.exit(0)

entries = {}
for kind, which in WORK:
    w = f"{kind}/{which}"
    if args.only and w not in args.only:
        continue
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--root", args.root, "--steps", str(args.steps), "--child", w],
                       capture_output=True, text=True, timeout=args.timeout)
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
    if r.returncode != 0 or not line:
        sys.exit(f"{w}: child failed ({r.returncode}): {r.stderr[-800:]}")
    key = w if args.steps == 40 else f"{w}@{args.steps}steps"          # (other step counts are workloads of their own in the file)
    entries[key] = json.loads(line[-1][7:])["ms"]
    print(f"{args.label:8s} {key:24s} {entries[key]:9.3f} ms")

if args.out:
    doc = json.load(open(args.out)) if os.path.exists(args.out) else {"runs": {}, "summary": {}}
    doc["runs"].setdefault(args.label, []).append(entries)
    doc["summary"] = {}
    for label, runs in doc["runs"].items():
        for w in sorted({k for r in runs for k in r}):
            vals = [r[w] for r in runs if w in r]
            doc["summary"].setdefault(w, {})[label] = dict(median_ms=statistics.median(vals), spread_ms=max(vals) - min(vals), runs=len(vals))
    with open(args.out, "w") as fh:
        json.dump(doc, fh, indent=1, sort_keys=True)
    for w, by in sorted(doc["summary"].items()):
        print(w, {k: (round(v["median_ms"], 3), round(v["spread_ms"], 3)) for k, v in by.items()})
