"""The row-banded "same" convolution (usf_conv2d_same_band_f32, usflows_amd/csrc/usf_conv_band.hip), launch by launch: the
case table in the style of tests/conv_kernel_cases.py, whose builder, fp64 / fp32 statements, checker and planted defects it
uses unchanged.  Importable without a GPU; tests/test_conv_band_cpu.py proves the table's coverage from the plan's answers
(usf_conv2d_same_band_variant), tests/test_conv_band_kernels_gpu.py launches every row.

A row: (name, entry, B, cin, cout, H, W, ks, band_rows, opts)
  entry      plain / ctx
  band_rows  the caps the SAME inputs are launched with (0: the plan's own band); every launch of a row must give the same bits
  opts       option preset of conv_kernel_cases.OPTS
The inputs of a row do not depend on B or band_rows (conv_kernel_cases.data draws sample-sequentially from a key without them).
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import conv_kernel_cases as K  # noqa: E402
from conv_kernel_cases import (Case, check, data, forward, guarded, measure, reference, bits, planes as pack,  # noqa: E402,F401
                               GUARD, MARGIN, SENTINEL_BITS, U, sentinel)

DEFECTS = ("tap_dropped", "in_mul_neighbour")      # conv_kernel_cases.forward's switches a multi-band case must catch
BAND_ROWS = (0, 1, 2, 5, 16)                       # the caps the table draws from
# max over this table of |fp32 statement - fp64 statement| / (U * A), measured on a CPU the way conv_kernel_cases measured its
# own 5.002: 5.324 (plain_64_64_17x17_k1: 64 terms at kernel 1; per entry plain 5.32, ctx 3.18) -- above conv_kernel_cases.K32 =
# 5.1, so this module has its own constant, rounded up in the second digit as that module rounds.
# tests/test_conv_band_cpu.py asserts that the fp32 statement stays inside it; the device is held to BOUND * U * A per element
K32 = 5.4
BOUND = MARGIN * K32

ROWS = [
    # 17 x 17 (289 pixels, odd width): the base shape, every cap
    ("plain_3_17_17x17", "plain", 2, 3, 17, 17, 17, 3, (0, 1, 2, 5, 16), "p2"),
    ("ctx_9_32_17x17", "ctx", 2, 9, 32, 17, 17, 3, (0, 1, 2, 5, 16), "c0"),
    ("ctx_1_3_17x17", "ctx", 2, 1, 3, 17, 17, 3, (0, 5), "c1"),
    ("plain_1_1_17x17", "plain", 2, 1, 1, 17, 17, 3, (0, 2), "p3"),
    ("plain_32_64_17x17", "plain", 2, 32, 64, 17, 17, 3, (0, 5, 16), "p1"),
    ("ctx_32_64_17x17", "ctx", 1, 32, 64, 17, 17, 3, (0, 5), "c1"),
    # 527 groups on 256 compute units: every block walks through edge and interior bands of different samples (stale halo rows)
    ("plain_32_32_17x17_stale", "plain", 31, 32, 32, 17, 17, 3, (1, 0), "p0"),
    ("ctx_9_17_17x17_stale", "ctx", 31, 9, 17, 17, 17, 3, (1, 2), "c0"),
    # kernel 1: no halo
    ("plain_64_64_17x17_k1", "plain", 2, 64, 64, 17, 17, 1, (0, 1, 5), "p0"),
    ("ctx_9_17_17x17_k1", "ctx", 31, 9, 17, 17, 17, 1, (1, 16), "c0"),
    # narrow and wide maps, one pixel wide (W = 1 has no magic-number division)
    ("plain_9_17_52x5", "plain", 2, 9, 17, 52, 5, 3, (0, 2, 5, 16), "p2"),
    ("ctx_3_32_52x5", "ctx", 2, 3, 32, 52, 5, 3, (0, 2), "c1"),
    ("ctx_3_64_5x64", "ctx", 2, 3, 64, 5, 64, 3, (0, 1, 2), "c0"),
    ("plain_9_64_5x64", "plain", 2, 9, 64, 5, 64, 3, (0, 1, 2), "p3"),
    ("plain_5_5_300x1", "plain", 2, 5, 5, 300, 1, 3, (0, 5), "p0"),
    # the shapes of MNIST and CIFAR at 32 -> 32 with the plan's own band (12 and 10 rows), once each
    ("plain_32_32_28x28", "plain", 1, 32, 32, 28, 28, 3, (0,), "p0"),
    ("ctx_32_32_32x32", "ctx", 2, 32, 32, 32, 32, 3, (0,), "c0"),
    # ... and their first layers (few input channels: a 16-row band fits): 32 x 32 patches in full last bands
    ("plain_3_32_32x32", "plain", 1, 3, 32, 32, 32, 3, (16, 5), "p2"),
    ("ctx_1_32_32x32", "ctx", 1, 1, 32, 32, 32, 3, (16, 2), "c1"),
    # ... and 32 x 32 patches in a ragged last band (28 = 16 + 12 rows)
    ("plain_1_32_28x28", "plain", 1, 1, 32, 28, 28, 3, (0, 16), "p3"),
    ("ctx_3_17_28x28", "ctx", 1, 3, 17, 28, 28, 3, (16,), "c0"),
    # the largest map: 4-row bands, 16 of them; 64 -> 64 at kernel 1: 8-row bands (register-bound)
    ("plain_32_32_64x64", "plain", 1, 32, 32, 64, 64, 3, (0,), "p1"),
    ("plain_64_64_32x32_k1", "plain", 1, 64, 64, 32, 32, 1, (0,), "p2"),
    # 256 pixels and fewer: held against usf_conv2d_same_f32 / _ctx_f32 on the same inputs
    ("small_plain_16_32_7x7", "plain", 5, 16, 32, 7, 7, 3, (0, 2), "p0"),
    ("small_ctx_5_7_8x8", "ctx", 3, 5, 7, 8, 8, 3, (0, 5), "c0"),
    ("small_plain_32_32_16x16", "plain", 3, 32, 32, 16, 16, 3, (0, 5), "p2"),
]

# refused shapes (usf_conv2d_same_band_fits == 0; the entry point answers 1): (cin, cout, H, W, ks)
REFUSED = [(65, 8, 17, 17, 3), (8, 65, 17, 17, 3), (8, 8, 5, 65, 3), (8, 8, 17, 241, 3), (8, 8, 64, 65, 1), (8, 8, 4097, 1, 1),
           (8, 8, 17, 17, 4), (8, 8, 17, 17, 5), (8, 8, 17, 17, 7), (64, 64, 32, 32, 3), (48, 48, 32, 32, 3)]
# ... and one whose best band has 3 rows (40 -> 40 at 32 x 32: 112 896 B of weights leave 203 image positions of 240 B)
REFUSED_3_ROWS = (40, 40, 32, 32, 3)

# the plan's figures of the issue's table: (cin, cout, H, W, ks) -> (weight bytes, best band, bands)
PLAN_FIGURES = {
    (1, 32, 28, 28, 3): (19968, 28, 1),
    (32, 32, 28, 28, 3): (56832, 12, 3),
    (32, 32, 32, 32, 3): (56832, 10, 4),
    (32, 32, 64, 64, 3): (56832, 4, 16),
    (64, 64, 32, 32, 1): (27648, 8, 4),
}


def _case(row):
    name, entry, B, cin, cout, H, W, ks, band_rows, opts = row
    assert all(b in BAND_ROWS for b in band_rows), name
    c = K._case((name, entry, B, cin, cout, H, W, ks, "", opts, (0,) * 6))
    c.band_rows = tuple(band_rows)
    return c


def cases():
    return [_case(r) for r in ROWS]


def band_kinds(H, rb):
    """the kinds of band a sample of H rows has at rb rows per band"""
    n = (H + rb - 1) // rb
    if n == 1:
        return {"only"}
    return {"first", "ragged_last" if H % rb else "last"} | ({"interior"} if n > 2 else set())
