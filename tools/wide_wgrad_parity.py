#!/usr/bin/env python3
"""profiles/wide_wgrad_parity.md from the figures tests/test_wide_wgrad_gpu.py prints:

    python -m pytest tests/test_wide_wgrad_gpu.py -q -s > wide.log && python tools/wide_wgrad_parity.py wide.log > profiles/wide_wgrad_parity.md

Per shape and batch: the worst of the forms run -- the kernel's error against fp64 over max|ref| (the test's bound is 2e-6) and the
error of a plain fp32 CPU computation (torch.nn.grad.conv2d_weight) of the same gradient in the same unit."""
import re
import sys

worst = {}
for line in open(sys.argv[1]):
    m = re.search(r"\((\d+, \d+, \d+, \d+, \d+)\) B=(\d+) (\w+) (dW|db): max\|ref\| (\S+) err (\S+) \((\S+) rel\) fp32-cpu err (\S+)", line)
    if not m:
        continue
    shape, B, form, what, scale, err, rel, e32 = m.groups()
    key = (tuple(int(v) for v in shape.split(", ")), int(B), what)
    if key not in worst or float(rel) > worst[key][0]:
        worst[key] = (float(rel), form, float(scale), float(e32))
top = max(v[0] for v in worst.values())
print("# usf_conv_wgrad_wide_f32 against fp64 (tests/test_wide_wgrad_gpu.py, one MI355X)\n")
print("Made by tools/wide_wgrad_parity.py from the test's printed figures.  Per shape `(cin, cout, H, W, ks)` and batch: the worst of")
print("the forms run (plain, mask + ReLU, pre_sub + leaky 0.1, no db) -- its error against fp64 relative to max|ref| (the test's bound")
print("is 2e-6), and beside it the error of a plain fp32 CPU computation of the same gradient (`torch.nn.grad.conv2d_weight`) against")
print(f"fp64 on the same inputs, in the same unit.  The worst case of all is {top:.1e}: the bound of the 64-pixel kernel's test holds")
print("unchanged.\n")
print("| shape | B | dW: kernel err / max ref | dW: fp32 CPU err / max ref | worst form | db: kernel err / max ref |")
print("|---|---|---|---|---|---|")
for (shape, B, what), v in sorted(worst.items()):
    if what == "dW":
        d = worst[(shape, B, "db")] if (shape, B, "db") in worst else (float("nan"),)
        print(f"| {shape} | {B} | {v[0]:.2e} | {v[3] / v[2]:.2e} | {v[1]} | {d[0]:.2e} |")
