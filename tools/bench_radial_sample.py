#!/usr/bin/env python3
"""``Flow.sample`` of the live MNIST flow (bench.py's mnist_live: [16,7,7], 15 blocks, 3 gated layers, prior_scale 1.0) over its
radial base -- the ``LogNormal(6, .35)`` of the live configuration and a ``GammaMM`` x 20 (p = 1) -- at 65 536 rows and at 100
rows: the sampling HEAD alone (``Flow._radial_sample_image``: from this commit on one usf_radial_sample_norm_f32 launch, before it
the norm distribution's own ``sample`` plus usf_radial_sample_f32) and the whole call.

One run measures ONE checkout and appends its entries to the JSON file; the comparison is made by running this same file
against a parent checkout on the same box, the two alternating, two runs each:

    python3 tools/bench_radial_sample.py --label this --out profiles/radial_sample_bench.json
    python3 tools/bench_radial_sample.py --root <parent checkout> --label parent --out profiles/radial_sample_bench.json    (and again)

Clock: the host clock around calls that end in a device synchronise; every shape is warmed up, then calls are repeated until
the timed window holds at least ``--window`` seconds.  The file then holds, per label and workload, the median over the runs
and the spread between the runs of one label: a difference between the labels means something where it exceeds that spread.
Prints the summary."""
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
ap.add_argument("--bases", nargs="+", default=["lognormal", "gammamm"])
ap.add_argument("--rows", nargs="+", type=int, default=[65536, 100])
ap.add_argument("--window", type=float, default=0.5, help="least seconds of timed work per figure")
ap.add_argument("--timeout", type=int, default=300, help="seconds per child process")
ap.add_argument("--out", default=None)
ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
args = ap.parse_args()
args.root = os.path.abspath(args.root)


def child(base_kind):
    """every figure of one base, in the checkout --root"""
    sys.path.insert(0, args.root)
    import torch
    import bench
    from usflows_amd import distributions as UD
    from usflows_amd.flows import USFlow
    from usflows_amd.networks import ConvNet2D
    cfg = bench.IMAGE_CONFIGS["mnist_live"]
    dims = list(cfg["in_dims"])
    torch.manual_seed(0)
    if base_kind == "lognormal":
        nd = UD.LogNormal(loc=torch.ones([1]) * 6, scale=torch.ones([1]) * .35, device="cpu")
    else:
        nd = UD.GammaMM(concentration=1 + torch.rand([20]) * 75, rate=0.05 + torch.rand([20]), mixture_weights=torch.ones([20]) / 20,
                        device="cpu")
    base = UD.RadialDistribution(device="cpu", p=float("1"), loc=torch.zeros(dims), norm_distribution=nd)
    flow = USFlow(base, dims, cfg["blocks"], ConvNet2D, dict(cfg["cond"]), prior_scale=cfg["prior_scale"],
                  householder=cfg["householder"], affine_conjugation=True)
    bench._condition_image_flow(flow, seed=0)
    flow = flow.to("cuda:0")
    dev = torch.device("cuda:0")

    def timed(fn):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        n, t0 = 0, time.perf_counter()
        while True:
            fn()
            n += 1
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            if dt >= args.window and n >= 5:
                return dt / n * 1e3, n

    out = {}
    with torch.no_grad():
        for rows in args.rows:
            ms_h, n_h = timed(lambda: flow._radial_sample_image((rows,), dev, 11, 0))
            ms_w, n_w = timed(lambda: flow.sample([rows], seed=11))
            xs = flow.sample([rows], seed=11)
            assert xs.shape == (rows, *dims) and bool(torch.isfinite(xs).all()), "the samples are not finite"
            out[f"head/{rows}"] = dict(ms=round(ms_h, 4), calls=n_h)
            out[f"sample/{rows}"] = dict(ms=round(ms_w, 4), calls=n_w)
    print(json.dumps(out))


def measure(base_kind):
    cmd = [sys.executable, os.path.abspath(__file__), "--root", args.root, "--window", str(args.window), "--rows",
           *[str(r) for r in args.rows], "--child", base_kind]
    r = subprocess.run(cmd, cwd=args.root, capture_output=True, text=True, timeout=args.timeout)
    if r.returncode != 0:
        raise RuntimeError(f"the measurement of {base_kind} failed (rc {r.returncode}): {r.stderr[-800:]}")
    return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])


def main():
    if args.child:
        return child(args.child)
    entries = []
    for b in args.bases:
        for k, v in measure(b).items():
            entries.append(dict(label=args.label, workload=f"{k}/{b}", **v))
    out = dict(what="mnist_live-shaped flow over a radial base (p = 1): Flow.sample ms per call, the sampling head alone "
                    "(head/<rows>/<base>) and the whole call (sample/<rows>/<base>); host clock around synchronised calls", runs=[])
    if args.out and os.path.exists(args.out):
        out = json.load(open(args.out))
    out["runs"].extend(entries)
    groups = {}
    for e in out["runs"]:
        groups.setdefault(f"{e['label']}/{e['workload']}", []).append(e)
    out["summary"] = {k: dict(median_ms=round(statistics.median(e["ms"] for e in v), 4), runs=len(v),
                              spread=round((max(e["ms"] for e in v) - min(e["ms"] for e in v)) / statistics.median(e["ms"] for e in v), 4))
                      for k, v in groups.items()}
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(json.dumps(out, indent=1) + "\n")
    print(json.dumps(out["summary"]))


if __name__ == "__main__":
    main()
