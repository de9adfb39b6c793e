#!/usr/bin/env python3
"""Inference and training of the image flows the reference's hyper-parameter search draws at ``kernel_size: 4``
(experiments/mnist/mnist_usflow_hyperopt.yaml: [16, 7, 7], CondConvNet2D, soft training, padding="same": one zero before the
image and two after), with the knob ``conv_k4`` on against a parent checkout (torch's convolution and autograd there), the
untouched kernel_size 3 twin as the control, and two 4 x 4 convolutions alone against F.conv2d.  The method of tools/bench_conv5.py.

One run measures ONE checkout under ONE value of the knob and appends its entries to the JSON file (the method of
tools/bench_image_wide.py); this commit and a parent checkout alternate on one box, two or three runs each:

    python3 tools/bench_conv4.py --root <parent checkout> --label parent --out profiles/conv4_bench.json   (a checkout without the knob)
    python3 tools/bench_conv4.py --knob 1 --label on  --out profiles/conv4_bench.json                      (and again, both)

  logprob65536/<flow>   log_prob of 65 536 rows with a per-row context: ms, median of the timed calls
  logprob100/<flow>     the same at the 100 rows the reference evaluates in (the replayed small-batch form): ms
  fit32/<flow>          Flow.fit with Adam at batch 32 on resident rows (the replayed step): ms per step
  fit1024/<flow>        the same at batch 1024
  conv/<cin>_<cout>_<H>x<W>/hip | torch   one 4 x 4 convolution of 4096 samples on usf_conv2d_same_f32 | F.conv2d: ms
                        (32 -> 32 keeps its weights in the LDS, 64 -> 64 streams them)
Flows: k4c32 / k4c64 = 5 blocks, CondConvNet2D(kernel_size=4, c_hidden 32 / 64, 3 gated layers, layer norm), radial LogNormal
base; k3c32 = the same at kernel_size 3.  (k4c64's training runs under torch autograd on a parent checkout or with the knob off: a
GatedConv of 64 channels has a 1 x 1 convolution of 128 outputs, which the knob runs in two halves.)  Prints the summary: per label and workload the median over the runs and their spread."""
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
ap.add_argument("--knob", type=int, default=1, help="conv_k4 (ignored by a checkout that has no such knob)")
ap.add_argument("--only", nargs="+", default=None)
ap.add_argument("--timeout", type=int, default=200, help="seconds per child process")
ap.add_argument("--out", default=None)
ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
args = ap.parse_args()

FLOWS = {"k4c32": (4, 32), "k4c64": (4, 64), "k3c32": (3, 32)}
CONVS = [(32, 32, 7, 7), (64, 64, 7, 7)]
WORK = [f"{k}/{f}" for f in FLOWS for k in ("logprob65536", "logprob100")] + \
    [f"{k}/{f}" for f in FLOWS for k in ("fit32", "fit1024")] + [f"conv/{a}_{b}_{h}x{w}" for a, b, h, w in CONVS]


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
    from usflows_amd import distributions as UD
    from usflows_amd.config import config
    from usflows_amd.flows import USFlow
    from usflows_amd.networks import CondConvNet2D
    warnings.simplefilter("ignore")
    if "conv_k4" in config._KNOBS:
        config.conv_k4 = bool(args.knob)
    dev = "cuda:0"
    kind, which = work.split("/", 1)
    out = {}
    if kind == "conv":
        import torch.nn.functional as F
        from usflows_amd import _ext
        shape, hw = which.rsplit("_", 1)
        cin, cout = (int(v) for v in shape.split("_"))
        H, W = (int(v) for v in hw.split("x"))
        g = torch.Generator().manual_seed(0)
        x = torch.randn(4096, cin, H, W, generator=g).to(dev)
        w = (torch.randn(cout, cin, 4, 4, generator=g) / (4 * cin ** 0.5)).to(dev)
        b = torch.randn(cout, generator=g).to(dev)
        out["torch"] = timed(lambda: F.conv2d(x, w, b, padding="same"), 5, 30)
        if _ext.load().usf_conv2d_same_fits(cin, cout, H, W, 4) >= 1:            # (0 on a checkout whose kernels do not take ks = 4)
            planes = _ext.conv2d_weight_planes(w)
            out["hip"] = timed(lambda: _ext.conv2d_same(x, planes, cout, 4, bias=b), 5, 30)
    else:
        ks, ch = FLOWS[which]
        dims = [16, 7, 7]
        torch.manual_seed(0)
        base = UD.RadialDistribution(device="cpu", p=1.0, loc=torch.zeros(dims),
                                     norm_distribution=UD.LogNormal(loc=torch.ones([1]) * 6, scale=torch.ones([1]) * .35, device="cpu"))
        cond = dict(c_in=16, c_hidden=ch, num_layers=3, padding="same", kernel_size=ks, normalize_layers=True, gating=True)
        flow = USFlow(base, dims, 5, CondConvNet2D, cond, prior_scale=1.0, householder=1, affine_conjugation=True, soft_training=True).to(dev)
        if kind.startswith("fit"):
            batch, steps = int(kind[3:]), 30
            n = batch * steps
            data = torch.rand(n, *dims, generator=torch.Generator().manual_seed(1))
            ds = torch.utils.data.TensorDataset(data, torch.zeros(n))
            kw = dict(optim=torch.optim.Adam, optim_params=dict(lr=1e-5), batch_size=batch, shuffle=False, device=torch.device(dev))
            flow.fit(ds, epochs=1, **kw)                               # warm-up: plans, capture
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            flow.fit(ds, epochs=2, **kw)
            torch.cuda.synchronize()
            print("RESULT " + json.dumps({"ms": (time.perf_counter() - t0) * 1e3 / (2 * steps)}))
            return
        rows = int(kind[len("logprob"):])
        x = torch.rand(rows, *dims, device=dev)
        ctx = 2.0 * torch.rand(rows, 1, device=dev)
        with torch.no_grad():
            out["ms"] = timed(lambda: flow.log_prob(x, ctx), 6, 20 if rows > 1000 else 100)
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
        key = w if k == "ms" else f"{w}/{k}"
        entries[key] = v
        print(f"{args.label:8s} {key:36s} {v:9.3f} ms", flush=True)

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
