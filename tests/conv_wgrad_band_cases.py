"""The row-banded weight-gradient kernel usf_conv_wgrad_band_f32 (usflows_amd/csrc/usf_conv_wgrad_band.hip), launch by launch:
the case table, and with the method of tests/image_grad_cases.py -- its data recipe (``wg_data``: exact zeros, elements equal to
pre_sub, one dy channel in 16 scaled by 2^-24), its four FORMS, its fp64 statement with the magnitude sum A and its two fp32
statements (einsum; strictly sequential over the samples), its guarded buffers -- the checker.  Importable without a GPU and
without the library; tests/test_conv_wgrad_band_cpu.py proves the table's coverage from usf_conv_wgrad_band_variant's answers,
tests/test_conv_wgrad_band_gpu.py launches every row in every form.

Rows: (cin, cout, H, W, ks, band_rows, B, block cap).  band_rows 0: the plan's band; block cap 0: none, else the tuning knob
conv_wgrad_band_blocks for the launch (with two blocks each block walks the bands of several samples).
"""
import torch

from image_grad_cases import (FORMS, GUARD, MARGIN, SENTINEL_BITS, U, Case, bits, guarded, ratio, untouched, wg_data,  # noqa: F401
                              wg_forward)

CUS = 256
ROWS = [
    (1, 16, 17, 17, 3, 4, 3, 0),       # bands of 4, 4, 4, 4, 1: first, interior, last and a ragged last band of one row
    (32, 32, 28, 28, 3, 0, 5, 2),      # each block walks interior -> first -> last bands of several samples: the stale-halo walk
    (3, 32, 32, 32, 3, 0, 2, 0),
    (32, 3, 32, 32, 3, 0, 2, 0),
    (32, 64, 28, 28, 1, 0, 3, 0),      # the gate convolution
    (33, 17, 19, 15, 3, 5, 2, 0),      # channel counts off every tile size, odd W, ragged band
    (16, 16, 26, 10, 1, 0, 3, 0),      # the two-tile instantiation, whose spare waves split the position chunks
    (64, 64, 20, 20, 1, 0, 2, 0),
    (64, 64, 17, 17, 3, 0, 2, 0),      # the most tiles per wave
    (2, 2, 64, 64, 3, 0, 1, 0),        # 4096 pixels at W = 64
    # one row per remaining tiles-per-wave instantiation: 2, 4, 7, 8, 15, 19, 21, 28
    (32, 32, 17, 17, 1, 0, 3, 0),
    (64, 48, 13, 21, 1, 3, 2, 0),        # bands of 3, 3, 3, 3, 1 at kernel 1
    (48, 16, 17, 17, 3, 0, 2, 3),
    (16, 48, 18, 16, 3, 0, 2, 0),
    (32, 48, 17, 17, 3, 2, 2, 0),        # nine bands of two rows and less
    (64, 32, 17, 17, 3, 0, 3, 2),
    (48, 48, 17, 17, 3, 0, 2, 0),
    (64, 48, 17, 17, 3, 1, 2, 0),        # bands of ONE row: every x row staged is some band's halo
    # the plan's other regimes
    (16, 32, 29, 28, 3, 0, 130, 0),    # a batch that keeps the LDS-sized band: 15 + 14 rows, 88 KiB of LDS (above the 64 KiB a kernel gets unasked)
    (8, 24, 4, 64, 3, 0, 3, 0),        # one band: the whole map of four rows
    (3, 16, 18, 16, 3, 4, 110, 0),     # 550 groups on 512 blocks: the grid at its cap, two reduction rounds, ragged band of two rows
    (5, 7, 31, 1, 3, 0, 2, 0),         # W == 1: the column taps meet the pad column only
]
# shapes the entry point refuses: kernel 4 / 5, W > 64, H W > 4096, channels above 64, an image of which no four rows fit
REFUSED = [(16, 16, 20, 20, 4), (16, 16, 20, 20, 5), (16, 16, 4, 65, 3), (16, 16, 65, 64, 1), (65, 16, 20, 20, 3), (16, 65, 20, 20, 1),
           (64, 64, 64, 64, 3)]
SMALL_MAP = (12, 16, 16, 16, 3, 5)     # (cin, cout, H, W, ks, B): the largest map usf_conv_wgrad_wide_f32 serves too

# max over the table (every row, every form) of |fp32 statement - fp64 statement| / (U * A), measured on a CPU
# (``measure_K`` below; tests/test_conv_wgrad_band_cpu.py asserts that the fp32 statements stay inside), rounded up in the
# second digit; the row that set each.  The larger of the two fp32 statements: torch's einsum / sum and a strictly sequential
# accumulation over the samples.
K = {
    "dW": 2.7,         # 2.616  64to32_17x17_k3_rb0_B3_cap2_presub_leaky (einsum)
    "db": 0.34,        # 0.337  64to48_13x21_k1_rb3_B2_presub_leaky (sum)
}
# the suite's max-norm bound for weight gradients, max |err| <= 2e-6 max |ref|: asserted here as well, the CPU fp32 statements
# stay under 1e-6 on every row (the worst: 6.1e-7 for dW, 3.5e-7 for db; profiles/conv_wgrad_band_parity.md)
MAXNORM = 2e-6


def name_of(row):
    cin, cout, H, W, ks, rb, B, cap = row
    return f"{cin}to{cout}_{H}x{W}_k{ks}_rb{rb}_B{B}" + (f"_cap{cap}" if cap else "")


def case(row, form):
    cin, cout, H, W, ks, rb, B, cap = row
    c = Case(name=f"{name_of(row)}_{form}", row=tuple(row), B=B, cin=cin, cout=cout, H=H, W=W, ks=ks, band_rows=rb, cap=cap, form=form)
    c.update(FORMS[form])
    return c


def cases():
    return [case(r, f) for r in ROWS for f in FORMS]


class block_cap:
    """the library's tuning knob conv_wgrad_band_blocks for the duration of a block (0: no cap, its default)"""

    def __init__(self, lib, cap):
        self.lib, self.cap = lib, int(cap)

    def __enter__(self):
        self.old = self.lib.usf_get_tuning(b"conv_wgrad_band_blocks", 0)
        assert self.lib.usf_set_tuning(b"conv_wgrad_band_blocks", self.cap) == 0

    def __exit__(self, *exc):
        assert self.lib.usf_set_tuning(b"conv_wgrad_band_blocks", int(self.old)) == 0


def fp32_ratios(c, d=None):
    """(worst |fp32 - fp64| / (U A) over dW, the same over db, max-norm figure of dW, of db) of the two fp32 statements on the CPU,
    the larger of the two each"""
    d = d or wg_data(c)
    r64 = wg_forward(c, d, torch.float64)
    out = [0.0, 0.0, 0.0, 0.0]
    for mode in ("einsum", "seq"):
        r32 = wg_forward(c, d, torch.float32, mode=mode)
        out[0] = max(out[0], ratio(r32.dW, r64.dW, r64.A_dW))
        out[1] = max(out[1], ratio(r32.db, r64.db, r64.A_db))
        out[2] = max(out[2], maxnorm(r32.dW, r64.dW))
        out[3] = max(out[3], maxnorm(r32.db, r64.db))
    return tuple(out)


def measure_K():
    """how K was measured: {"dW": (worst ratio, case name), "db": ...} over every row and form"""
    worst = {"dW": (0.0, ""), "db": (0.0, "")}
    for c in cases():
        rW, rb, _, _ = fp32_ratios(c)
        worst["dW"] = max(worst["dW"], (rW, c.name))
        worst["db"] = max(worst["db"], (rb, c.name))
    return worst


def maxnorm(got, ref64):
    """max |err| / max |ref|"""
    return (got.double() - ref64).abs().max().item() / max(ref64.abs().max().item(), 1e-30) if ref64.numel() else 0.0


def check(what, buf, ref64, A64, family, lo=GUARD):
    """every finding of one output's guarded buffer against the fp64 statement; [] = it passes.  Per element
    |got - fp64| <= MARGIN * K[family] * U * A, the suite's max-norm bound next to it, the sentinels on both sides intact"""
    n = ref64.numel()
    out = []
    s = torch.tensor([SENTINEL_BITS], dtype=torch.int32, device=buf.device)
    if not bool((bits(buf[:lo]) == s).all()):
        out.append(f"written in front of {what}")
    if not bool((bits(buf[lo + n:]) == s).all()):
        out.append(f"written behind {what}")
    got = buf[lo:lo + n].view(ref64.shape)
    left = bits(got) == s
    if bool(left.any()):
        out.append(f"{int(left.sum())} elements of {what} left unwritten")
    if not bool(torch.isfinite(got).all()):
        out.append(f"non-finite values in {what}")
        return out
    bound = MARGIN * K[family]
    err = (got.double() - ref64).abs()
    over = err > bound * U * A64
    if bool(over.any()):
        i = int(torch.where(over, err / (U * A64).clamp_min(1e-300), torch.zeros_like(err)).argmax())
        out.append(f"{int(over.sum())} elements of {what} over {bound:.1f} U A; worst at flat index {i}: got {got.flatten()[i].item()!r}, "
                   f"fp64 {ref64.flatten()[i].item()!r}, A {A64.flatten()[i].item()!r}")
    if maxnorm(got, ref64) > MAXNORM:
        out.append(f"max-norm bound of {what}: {maxnorm(got, ref64):.3e} > {MAXNORM}")
    return out
