#!/usr/bin/env python3
"""Training of image flows whose feature maps have more than 256 pixels -- MNIST [1, 28, 28] and CIFAR [3, 32, 32] without
space-to-depth -- with the knob ``train_band`` on (usf_conv2d_same_band_f32 for forward and data gradient, usf_conv_wgrad_band_f32
for the weight gradients) against a parent checkout (torch autograd + MIOpen there), and untouched workloads on both as controls.

One run measures ONE checkout under ONE value of the knob and appends its entries to the JSON file (the method of
tools/bench_conv_band.py); this commit and a parent checkout alternate on one MI355X, two runs each:

    python3 tools/bench_image_band_train.py --root <parent checkout> --label parent --out profiles/image_band_train_bench.json
    python3 tools/bench_image_band_train.py --knob 1 --label on --out profiles/image_band_train_bench.json          (and again, both)

  fit32/<flow>, fit1024/<flow>   Flow.fit with Adam at batch 32 / 1024: ms per step = (a fit of 3 epochs - a fit of 1 epoch) / the
                                 steps of 2 epochs, so that what a fit call costs once (capture, upload) drops out
  step4096/<flow>                one eager training step (log_prob, loss, backward) of 4096 rows: ms, median of the timed steps
  launches32/<flow>              library launches of ONE eager batch-32 pass (log_prob + backward); aten32/<flow>: the torch operators
                                 the same pass dispatches (on the parent the conditioners' convolutions are among them)
  controls: fit32/control7 ([16, 7, 7]) and fit32/control14 ([4, 14, 14]) -- maps the knob does not touch -- and logprob8192/mnist,
  the inference path, which must not move.
Flows: 5 blocks, ConvNet2D(c_hidden 32, 3 gated layers, layer norm, kernel 3), radial LogNormal base, prior_scale 1.0 (the flows of
profiles/conv_band_bench.json).  Prints the summary: per label and workload the median over the runs and the spread between the
runs of one label."""
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
ap.add_argument("--knob", type=int, default=1, help="train_band (ignored by a checkout that has no such knob)")
ap.add_argument("--only", nargs="+", default=None)
ap.add_argument("--timeout", type=int, default=300, help="seconds per child process")
ap.add_argument("--out", default=None)
ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
args = ap.parse_args()

FLOWS = {"mnist": [1, 28, 28], "cifar": [3, 32, 32], "control7": [16, 7, 7], "control14": [4, 14, 14]}
WORK = [f"{k}/{f}" for f in ("mnist", "cifar") for k in ("fit32", "fit1024", "step4096", "launches32")] + \
    ["fit32/control7", "fit32/control14", "logprob8192/mnist"]


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
    if "train_band" in config._KNOBS:
        config.train_band = bool(args.knob)
    dev = "cuda:0"
    kind, which = work.split("/", 1)
    dims = FLOWS[which]
    torch.manual_seed(0)
    base = UD.RadialDistribution(device="cpu", p=1.0, loc=torch.zeros(dims),
                                 norm_distribution=UD.LogNormal(loc=torch.ones([1]) * 6, scale=torch.ones([1]) * .35, device="cpu"))
    cond = dict(c_in=dims[0], c_hidden=32, num_layers=3, padding="same", kernel_size=3, normalize_layers=True, gating=True)
    flow = USFlow(base, dims, 5, ConvNet2D, cond, prior_scale=1.0, lu_transform=1, householder=0, affine_conjugation=True).to(dev)
    out = {}

    def sync_time(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    if kind.startswith("fit"):
        batch = int(kind[3:])
        steps = 12 if batch <= 32 else 4
        data = torch.rand(batch * steps, *dims, generator=torch.Generator().manual_seed(1))
        ds = torch.utils.data.TensorDataset(data, torch.zeros(data.shape[0]))

        def fit(epochs):
            return flow.fit(ds, optim=torch.optim.Adam, optim_params=dict(lr=1e-6), batch_size=batch, shuffle=False,
                            device=torch.device(dev), epochs=epochs)
        fit(1)                                                     # (first sighting: planes, probes, the allocator)
        ts = []
        for _ in range(3):
            t1, t3 = sync_time(lambda: fit(1)), sync_time(lambda: fit(3))
            ts.append((t3 - t1) / (2 * steps))
        out["ms"] = statistics.median(ts)
    elif kind == "step4096":
        x = torch.rand(4096, *dims, device=dev)

        def step():
            for p in flow.parameters():
                p.grad = None
            (-flow.log_prob(x).mean()).backward()
        for _ in range(2):
            step()
        out["ms"] = statistics.median(sync_time(step) for _ in range(5))
    elif kind == "launches32":
        from torch.utils._python_dispatch import TorchDispatchMode
        x = torch.rand(32, *dims, device=dev)
        for _ in range(2):
            (-flow.log_prob(x).mean()).backward()
        n = {"lib": 0, "aten": 0}
        real = _ext._launch

        def counted(name, *a, **k):
            n["lib"] += 1
            return real(name, *a, **k)
        _ext._launch = counted

        class Mode(TorchDispatchMode):
            def __torch_dispatch__(self, func, types, a=(), kw=None):
                n["aten"] += 1
                return func(*a, **(kw or {}))
        with Mode():
            (-flow.log_prob(x).mean()).backward()
        torch.cuda.synchronize()
        out["ms"], out["aten32"] = n["lib"], n["aten"]
    else:
        rows = int(kind[len("logprob"):])
        x = torch.rand(rows, *dims, device=dev)
        with torch.no_grad():
            for _ in range(4):
                flow.log_prob(x)
            out["ms"] = statistics.median(sync_time(lambda: flow.log_prob(x)) for _ in range(10))
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
