#!/usr/bin/env python3
"""profiles/channel_affine_bwd_parity.md from the figures tests/test_channel_affine_bwd_gpu.py prints:

    python3 -m pytest tests/test_channel_affine_bwd_gpu.py -q -s > log.txt;  python3 tools/channel_affine_bwd_parity.py log.txt
"""
import re
import sys

rows, emu = {}, []
for line in open(sys.argv[1]):
    m = re.match(r"\.*(\S+) (dW|db|dx): max\|ref\| \S+ err \S+ \((\S+) rel\)", line)
    if m:
        C = int(re.search(r"_C(\d+)_", m.group(1)).group(1))
        rows.setdefault(C, {}).setdefault(m.group(2), []).append((float(m.group(3)), m.group(1)))
    m = re.match(r"\.*(\S+): dW differs from the numpy statement by (\S+)", line)
    if m:
        emu.append(float(m.group(2)))
worst = max(v for by in rows.values() for vs in by.values() for v in vs)
print("# usf_channel_affine_bwd_f32 against fp64 (tests/test_channel_affine_bwd_gpu.py, one MI355X)\n")
print("Made by tools/channel_affine_bwd_parity.py from the test's printed figures: per channel count the worst case of each output --")
print("its largest error against fp64 relative to max|ref| (the test's bound is 2e-6) -- over every case of")
print(f"tests/channel_affine_bwd_cases.py with that C ({sum(len(by['dW']) for by in rows.values())} launches: B in 1, 3, 33 and more, P in 1, 49, 196, 256, both forms, capped grids,")
print(f"unaligned tensors).  The worst figure of all is {worst[0]:.2e} ({worst[1]}).  The numpy fp32 statement of the kernel's summation")
print(f"order (tests/channel_affine_bwd_cases.py `emulate`) stays under 1.5e-7 on the same cases on the CPU; on the device dW differs")
print(f"from it by at most {max(emu):.1e} over the {len(emu)} cases (0: the same bits).\n")
print("| C | cases | dW: worst err / max ref | case | db: worst | case | dx: worst | case |")
print("|---|---|---|---|---|---|---|---|")
for C in sorted(rows):
    by = rows[C]
    cells = []
    for k in ("dW", "db", "dx"):
        e, name = max(by[k])
        cells += [f"{e:.2e}", name]
    print(f"| {C} | {len(by['dW'])} | " + " | ".join(cells) + " |")
