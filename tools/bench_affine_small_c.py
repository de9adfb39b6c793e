#!/usr/bin/env python3
"""Training steps of the [4, 14, 14] flow of tools/bench_image_wide.py (the reference's experiments/mnist/mnist_usflow_gpu.yaml
at a servable width: 5 coupling blocks, ConvNet2D with c_hidden 16, 4 gated layers, layer norm, Householder 1, conjugation) with
the two routes this commit adds -- the affine blocks' backward on usf_channel_affine_bwd_f32 (knob affine_small_c) and the fused
gated tail above 64 pixels (knob gated_tail_wide) -- each alone and both together, against a parent checkout; and the untouched
[16, 7, 7] MNIST model as the regression check.

One run measures ONE checkout with ONE setting of the knobs and appends its entries to the JSON file; the comparison is made by
running this same file against a parent checkout on the same box, the labels alternating, two runs each:

    python3 tools/bench_affine_small_c.py --root <parent checkout> --label parent --out profiles/affine_small_c_bench.json
    python3 tools/bench_affine_small_c.py --knobs both            --out profiles/affine_small_c_bench.json
    python3 tools/bench_affine_small_c.py --knobs affine_small_c  --out profiles/affine_small_c_bench.json
    python3 tools/bench_affine_small_c.py --knobs gated_tail_wide --out profiles/affine_small_c_bench.json          (and again)
    python3 tools/bench_affine_small_c.py [--root <parent checkout> --label parent] --only fit32/mnist --steps 400 --out ...

--knobs sets BOTH knobs explicitly through USFLOWS_AMD_TUNE (the named ones on, the other off), whatever their defaults are; a
parent checkout does not know them and ignores them.  The label is "parent" or "this/<knobs>".

  fit32/<flow>      Flow.fit with Adam at batch 32 on resident rows (the replayed step): ms per step
  fit1024/wide      the same at the configuration file's batch of 1024
  step4096/wide     one training step (log_prob, backward) at 4096 rows: ms, median of the timed steps
  launches32/wide   kernel launches of ONE eager training pass (log_prob, backward inside Flow.fit's backward scope) at batch 32,
                    counted from the torch profiler's ordered device trace: all, and those of the named kernels

The file then holds, per label and workload, all runs, their median and the spread between them, and under "knobs" the verdict
for each knob alone: on by default only where parent - knob exceeds the larger of the two spreads at batch 32 AND at batch 1024.
Prints the summary."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

KNOBS = ("affine_small_c", "gated_tail_wide")
ap = argparse.ArgumentParser()
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))), help="the checkout to measure")
ap.add_argument("--label", default=None, help="default: this/<knobs>")
ap.add_argument("--knobs", default="both", choices=("both", "none") + KNOBS)
ap.add_argument("--steps", type=int, default=40)
ap.add_argument("--only", nargs="+", default=None, help="workloads to run (default: all but fit32/mnist), e.g. fit32/mnist")
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
WORK = ["fit32/wide", "fit1024/wide", "step4096/wide", "launches32/wide"]
NAMED = ("channel_affine_bwd", "channel_affine_kernel", "gated_tail", "conv_wgrad", "partial_sum", "affine_prep")


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
    elif kind.startswith("step"):
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
    else:
        from torch.profiler import ProfilerActivity, profile
        x = torch.rand(int(kind[8:]), *dims, device=dev)

        def one_pass():
            for p in flow.parameters():
                p.grad = None
            loss = -flow.log_prob(x).mean()
            with flow._fit_backward_scope():
                loss.backward()
            torch.cuda.synchronize()

        for _ in range(3):
            one_pass()
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            one_pass()
        names = [e.name for e in sorted(prof.events(), key=lambda e: e.time_range.start)
                 if str(e.device_type).endswith("CUDA") and "memcpy" not in e.name.lower() and "memset" not in e.name.lower()]
        out["launches"] = dict(all=len(names), **{k: sum(k in n_ for n_ in names) for k in NAMED})
    print("RESULT " + json.dumps(out))


if args.child:
    child(args.child)
    sys.exit(0)

here = os.path.abspath(args.root) == os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
label = args.label or ("this/" + args.knobs if here else "parent")
on = KNOBS if args.knobs == "both" else () if args.knobs == "none" else (args.knobs,)
env = dict(os.environ)
tune = [t for t in env.get("USFLOWS_AMD_TUNE", "").split(",") if t and t.split("=")[0] not in KNOBS]
env["USFLOWS_AMD_TUNE"] = ",".join(tune + [f"{k}={int(k in on)}" for k in KNOBS])
entries = {}
for w in args.only or WORK:
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--root", args.root, "--steps", str(args.steps), "--child", w],
                       capture_output=True, text=True, timeout=args.timeout, env=env)
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
    if r.returncode != 0 or not line:
        if w.startswith("launches") and r.returncode == 1:      # (a Python error under the profiler: the timings above are kept)
            print(f"{w}: child failed ({r.returncode}): {r.stderr[-400:]}", file=sys.stderr)
            continue
        sys.exit(f"{w}: child failed ({r.returncode}): {r.stderr[-800:]}")
    key = w if args.steps == 40 or w.startswith("launches") else f"{w}@{args.steps}steps"      # (other step counts are workloads of their own)
    res = json.loads(line[-1][7:])
    entries[key] = res.get("ms", res.get("launches"))
    print(f"{label:24s} {key:24s} {entries[key] if isinstance(entries[key], dict) else round(entries[key], 3)}")

if args.out:
    doc = json.load(open(args.out)) if os.path.exists(args.out) else {}
    doc.setdefault("what", "ms per training step (Flow.fit with Adam, replayed; one 4096-row step) and kernel launches of one eager "
                           "pass at batch 32, per label: a parent checkout and this commit with the named knobs on, the other off")
    doc.setdefault("runs", {}).setdefault(label, []).append(entries)
    doc["summary"], doc["launches"] = {}, {}
    for lb, runs in doc["runs"].items():
        for w in sorted({k for r in runs for k in r}):
            vals = [r[w] for r in runs if w in r]
            if isinstance(vals[0], dict):
                doc["launches"].setdefault(w, {})[lb] = vals[-1]
            else:
                doc["summary"].setdefault(w, {})[lb] = dict(median_ms=statistics.median(vals), spread_ms=max(vals) - min(vals), runs=len(vals))
    # each knob alone against the parent: on by default only where the gain exceeds the larger spread at batch 32 AND 1024
    doc["knobs"] = {}
    for k in KNOBS:
        verdict = {}
        for w in ("fit32/wide", "fit1024/wide"):
            by = doc["summary"].get(w, {})
            if "parent" in by and "this/" + k in by:
                gain = by["parent"]["median_ms"] - by["this/" + k]["median_ms"]
                noise = max(by["parent"]["spread_ms"], by["this/" + k]["spread_ms"])
                verdict[w] = dict(gain_ms=gain, larger_spread_ms=noise, beyond_spread=bool(gain > noise))
        if len(verdict) == 2:
            verdict["on_by_default"] = all(v["beyond_spread"] for v in verdict.values())
            doc["knobs"][k] = verdict
    with open(args.out, "w") as fh:
        json.dump(doc, fh, indent=1, sort_keys=True)
    for w, by in sorted(doc["summary"].items()):
        print(w, {k: (round(v["median_ms"], 3), round(v["spread_ms"], 3)) for k, v in by.items()})
    print("knobs", json.dumps(doc["knobs"]))
