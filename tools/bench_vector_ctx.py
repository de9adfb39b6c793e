#!/usr/bin/env python3
"""A vector context (ConditionalDenseNN with context_dim = 10) on the device path, on the cfg2-shaped model (D = 784, 32 coupling
blocks, hidden [256, 256]): log_prob at 65 536 rows and one training step (log_prob(x, ctx), backward of -mean) at 32 and at 4096
rows, HIP-event timed after warm-up, next to the same flow with context_dim = 1 (the untouched scalar-context instantiations).

One run measures ONE checkout and appends its entries to the JSON file; the comparison with the parent commit (where context_dim
= 10 runs the torch composite) is made by running this same file from a parent checkout on the same box, the two alternating:

    python3 tools/bench_vector_ctx.py --label this   --out profiles/vector_ctx_bench.json
    python3 <this file> --root <parent checkout> --label parent --out profiles/vector_ctx_bench.json      (and again, alternating)

The file then holds, per label and context_dim, the median of every run's rounds and the spread between runs.  The flow's
parameters are the synthetic generator's for context_dim = 1 with layers[1].weight redrawn as [h0, C] by this tool, so both
checkouts build the same model.  Prints the file's summary as one JSON line."""
import argparse
import json
import os
import statistics
import sys
import warnings

import torch

ap = argparse.ArgumentParser()
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))), help="the checkout to measure")
ap.add_argument("--label", default="this")
ap.add_argument("--rows", type=int, default=65536)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--iters", type=int, default=5)
ap.add_argument("--blocks", type=int, default=32)
ap.add_argument("--out", default=None)
args = ap.parse_args()
sys.path.insert(0, args.root)
sys.path.insert(0, os.path.join(args.root, "tests"))
from oracle import usflows_oracle as orc  # noqa: E402
from usflows_amd.flows import USFlow  # noqa: E402
from usflows_amd.networks import ConditionalDenseNN  # noqa: E402

DEV = torch.device("cuda:0")
D, HIDDEN = 784, [256, 256]


def build(C):
    spec = orc.FlowSpec(dim=D, coupling_blocks=args.blocks, hidden_dims=HIDDEN, householder=0, affine_conjugation=False)
    sd = orc.synth_state_dict(spec, seed=2)
    g = torch.Generator().manual_seed(20 + C)
    for k in [k for k in sd if k.endswith("conditioner.layers.1.weight")]:
        sd[k] = (torch.rand(HIDDEN[0], C, generator=g) * 2 - 1) / C ** 0.5
    base = torch.distributions.Laplace(torch.zeros(D, device=DEV), torch.ones(D, device=DEV))
    flow = USFlow(base, [D], args.blocks, ConditionalDenseNN,
                  dict(input_dim=D, context_dim=C, hidden_dims=HIDDEN, out_dim=D, nonlinearity=torch.nn.LeakyReLU(0.01)),
                  affine_conjugation=False, householder=0)
    res = flow.load_state_dict(sd, strict=False)
    assert not res.unexpected_keys, res.unexpected_keys
    return flow.to(DEV)


def timed(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / n


def main():
    assert torch.cuda.is_available(), "bench_vector_ctx.py measures on the GPU"
    entries = []
    for C in (10, 1):
        flow = build(C)
        g = torch.Generator().manual_seed(C)
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter("always")
            device_path = flow.engine() is not None
            work = {}
            for key, rows, train in (("log_prob", args.rows, False), ("train32", 32, True), ("train4096", 4096, True)):
                x = torch.rand(rows, D, generator=g).to(DEV)
                ctx = torch.rand(rows, C, generator=g).to(DEV)
                if train:
                    def fn(x=x, ctx=ctx):
                        for p in flow.parameters():
                            p.grad = None
                        (-flow.log_prob(x, ctx).mean()).backward()
                else:
                    def fn(x=x, ctx=ctx):
                        with torch.no_grad():
                            flow.log_prob(x, ctx)
                for _ in range(2):
                    fn()
                torch.cuda.synchronize()
                work[key] = fn
            ms = {k: [timed(f, args.iters) for _ in range(args.rounds)] for k, f in work.items()}
        entries.append(dict(label=args.label, context_dim=C, device_path=device_path,
                            composite_warning=any(issubclass(w.category, RuntimeWarning) for w in caught),
                            ms={k: round(statistics.median(v), 4) for k, v in ms.items()},
                            ms_rounds={k: [round(t, 4) for t in v] for k, v in ms.items()}))
        del flow
        torch.cuda.empty_cache()
    out = dict(model=f"cfg2-shaped: D={D}, {args.blocks} blocks, hidden {HIDDEN}", rows=args.rows, runs=[])
    if args.out and os.path.exists(args.out):
        out = json.load(open(args.out))
    out["runs"].extend(entries)
    # per (label, context_dim, workload): the median over the runs and the spread between them
    summary = {}
    for e in out["runs"]:
        for k, v in e["ms"].items():
            summary.setdefault(f"{e['label']}/C{e['context_dim']}/{k}", []).append(v)
    out["summary"] = {k: dict(median_ms=round(statistics.median(v), 4), runs=len(v),
                              spread=round((max(v) - min(v)) / statistics.median(v), 4)) for k, v in summary.items()}
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(json.dumps(out, indent=1) + "\n")
    print(json.dumps(out["summary"]))


if __name__ == "__main__":
    main()
