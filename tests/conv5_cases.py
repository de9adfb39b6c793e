"""The "same" convolution at ks = 5, launch by launch: the forward case table of tests/test_conv5_cpu.py and
tests/test_conv5_kernels_gpu.py.  Importable without a GPU and without the library.  What is general -- the case builder, the
data, the plane layout, the fp64 / fp32 statements, the guarded buffer and the checker -- is tests/conv_kernel_cases.py's;
only what ks = 5 adds is stated here.

A row has the format of conv_kernel_cases.ROWS: (name, entry, B, cin, cout, H, W, ks, knobs, opts, expect), entries plain / ctx,
  expect  (kernel, S, NB, CP, NCT, CTX) from usf_conv2d_same_variant at 256 compute units: kernel 1 = weights resident in the LDS
          (conv2d_same_bf16x3_kernel; NB = CP = NCT = 0), kernel 4 = weights streamed (conv2d_same_k5_stream_kernel; NB = 32-value
          k-blocks per slab, CP = padded input channels, NCT = slabs in the ring), kernel 0 = refused with -3, nothing launched.
Rows named *_a / *_b are the two batches of one shape: (a) one sample fewer than fit a group, so S is clipped to the batch
(B = 1 where one sample fits); (b) B = S (2 * 256 + k) + r, 0 < r < S (S = 1: B = 2 * 256 + k): blocks run three groups and two,
the last group is ragged, and the streamed kernel's ring is carried across groups.  Both batches draw the same samples, so (a)'s
outputs must be a bit-exact prefix of (b)'s.
"""
from conv_kernel_cases import _case, MARGIN  # noqa: F401

# max over this table of |fp32 statement - fp64 statement| / (U * A), measured on a CPU (tests/test_conv5_cpu.py prints it per
# entry), rounded up in the second digit.  The CPU test asserts that the fp32 statement stays inside it; the device is held to
# MARGIN * K32_5 * U * A per element.  It comes from the fp32 CPU statement, never from a kernel.  Measured: 3.545
# (k5_res_5_64_8x8_b; per entry plain 3.545, ctx 2.410).
K32_5 = 3.6

# (tag, entry, cin, cout, H, W, opts, k): the shapes with two batches each
FAMILIES = [
    # weights resident
    ("res_1_7_1x1", "plain", 1, 7, 1, 1, "p0", 1),               # every tap but the centre reads padding
    ("res_ctx_5_16_2x3", "ctx", 5, 16, 2, 3, "c0", 2),           # smaller than the kernel in both axes, not square
    ("res_16_16_7x7", "plain", 16, 16, 7, 7, "p1", 3),
    ("res_ctx_16_40_7x7", "ctx", 16, 40, 7, 7, "c1", 1),         # resident with exactly two samples
    ("res_5_64_8x8", "plain", 5, 64, 8, 8, "p2", 2),             # cp = 8: K 200 -> 224
    # weights streamed
    ("str_64_64_7x7", "plain", 64, 64, 7, 7, "p3", 1),           # slabs of a tap, 25 of them (odd)
    ("str_ctx_64_64_7x7", "ctx", 64, 64, 7, 7, "c1", 2),
    ("str_ctx_16_64_7x7", "ctx", 16, 64, 7, 7, "c0", 3),         # K 400 -> 416 = 6.5 slabs: the last slab is short
    ("str_64_64_8x8", "plain", 64, 64, 8, 8, "p0", 1),           # half-tap slabs, 50 of them (even)
    ("str_33_64_16x16", "plain", 33, 64, 16, 16, "p1", 1),       # cp = 40, K 1000 -> 1024 = 16 slabs (even), one sample per group
    ("str_ctx_64_7_7x7", "ctx", 64, 7, 7, 7, "c1", 2),           # one tile of output channels: eight row ranges
    ("str_64_16_8x8", "plain", 64, 16, 8, 8, "p2", 3),
    ("str_32_32_7x7", "plain", 32, 32, 7, 7, "p2", 1),           # K 800 = 12.5 slabs
    ("str_16_40_5x13", "plain", 16, 40, 5, 13, "p3", 2),         # three tiles of output channels: the second wave group has one
]


def generate_rows(probe):
    """probe(entry, B, cin, cout, H, W, ks, aligned, knobs) -> the answer dict of usf_conv2d_same_variant at 256 compute units"""
    rows = []

    def add(name, entry, B, cin, cout, H, W, opts):
        aligned = not ("xoff" in opts or "yoff" in opts)
        a = probe(entry, B, cin, cout, H, W, 5, aligned, "")
        exp = (a["kernel"], a["S"], a["NB"], a["CP"], a["NCT"], a["CTX"]) if a["kernel"] else (0, 0, 0, 0, 0, 0)
        rows.append((name, entry, B, cin, cout, H, W, 5, "", opts, exp))

    for tag, entry, cin, cout, H, W, opts, k in FAMILIES:
        best = probe(entry, 1 << 16, cin, cout, H, W, 5, True, "")["S"]
        add(f"k5_{tag}_a", entry, max(1, best - 1), cin, cout, H, W, opts)
        add(f"k5_{tag}_b", entry, best * (2 * 256 + k) + max(1, best // 2) if best > 1 else 2 * 256 + k, cin, cout, H, W, opts)
    add("k5_res_16_32_7x7_clipped", "plain", 3, 16, 32, 7, 7, "p0")            # the first kernel's 16 x 32 patch
    add("k5_res_16_16_7x7_x_offset", "plain", 50, 16, 16, 7, 7, "p0+xoff")
    add("k5_str_ctx_16_64_7x7_y_offset", "ctx", 23, 16, 64, 7, 7, "c0+yoff")
    add("k5_str_32_64_7x7_xy_offset", "plain", 10, 32, 64, 7, 7, "p2+xoff+yoff")
    # no plan holds 64 input channels of a 16 x 16 map (20 x 20 positions x 3 planes x 144 B = 172 800 B)
    add("k5_refused_64_64_16x16", "plain", 3, 64, 64, 16, 16, "p0")
    add("k5_refused_ctx_64_16_16x16", "ctx", 3, 64, 16, 16, 16, "c0")
    return rows


# ---- the table (generate_rows with the library's answers; tests/test_conv5_cpu.py holds the two equal) -------------------------
ROWS = [
    ("k5_res_1_7_1x1_a", "plain", 7, 1, 7, 1, 1, 5, "", "p0", (1, 7, 0, 0, 0, 0)),
    ("k5_res_1_7_1x1_b", "plain", 4108, 1, 7, 1, 1, 5, "", "p0", (1, 8, 0, 0, 0, 0)),
    ("k5_res_ctx_5_16_2x3_a", "ctx", 7, 5, 16, 2, 3, 5, "", "c0", (1, 7, 0, 0, 0, 1)),
    ("k5_res_ctx_5_16_2x3_b", "ctx", 4116, 5, 16, 2, 3, 5, "", "c0", (1, 8, 0, 0, 0, 1)),
    ("k5_res_16_16_7x7_a", "plain", 5, 16, 16, 7, 7, 5, "", "p1", (1, 5, 0, 0, 0, 0)),
    ("k5_res_16_16_7x7_b", "plain", 3093, 16, 16, 7, 7, 5, "", "p1", (1, 6, 0, 0, 0, 0)),
    ("k5_res_ctx_16_40_7x7_a", "ctx", 1, 16, 40, 7, 7, 5, "", "c1", (1, 1, 0, 0, 0, 1)),
    ("k5_res_ctx_16_40_7x7_b", "ctx", 1027, 16, 40, 7, 7, 5, "", "c1", (1, 2, 0, 0, 0, 1)),
    ("k5_res_5_64_8x8_a", "plain", 7, 5, 64, 8, 8, 5, "", "p2", (1, 7, 0, 0, 0, 0)),
    ("k5_res_5_64_8x8_b", "plain", 4116, 5, 64, 8, 8, 5, "", "p2", (1, 8, 0, 0, 0, 0)),
    ("k5_str_64_64_7x7_a", "plain", 1, 64, 64, 7, 7, 5, "", "p3", (4, 1, 2, 64, 2, 0)),
    ("k5_str_64_64_7x7_b", "plain", 1027, 64, 64, 7, 7, 5, "", "p3", (4, 2, 2, 64, 2, 0)),
    ("k5_str_ctx_64_64_7x7_a", "ctx", 1, 64, 64, 7, 7, 5, "", "c1", (4, 1, 2, 64, 2, 1)),
    ("k5_str_ctx_64_64_7x7_b", "ctx", 1029, 64, 64, 7, 7, 5, "", "c1", (4, 2, 2, 64, 2, 1)),
    ("k5_str_ctx_16_64_7x7_a", "ctx", 4, 16, 64, 7, 7, 5, "", "c0", (4, 4, 2, 16, 2, 1)),
    ("k5_str_ctx_16_64_7x7_b", "ctx", 2577, 16, 64, 7, 7, 5, "", "c0", (4, 5, 2, 16, 2, 1)),
    ("k5_str_64_64_8x8_a", "plain", 1, 64, 64, 8, 8, 5, "", "p0", (4, 1, 1, 64, 2, 0)),
    ("k5_str_64_64_8x8_b", "plain", 1027, 64, 64, 8, 8, 5, "", "p0", (4, 2, 1, 64, 2, 0)),
    ("k5_str_33_64_16x16_a", "plain", 1, 33, 64, 16, 16, 5, "", "p1", (4, 1, 2, 40, 2, 0)),
    ("k5_str_33_64_16x16_b", "plain", 513, 33, 64, 16, 16, 5, "", "p1", (4, 1, 2, 40, 2, 0)),
    ("k5_str_ctx_64_7_7x7_a", "ctx", 1, 64, 7, 7, 7, 5, "", "c1", (4, 1, 2, 64, 2, 1)),
    ("k5_str_ctx_64_7_7x7_b", "ctx", 1029, 64, 7, 7, 7, 5, "", "c1", (4, 2, 2, 64, 2, 1)),
    ("k5_str_64_16_8x8_a", "plain", 1, 64, 16, 8, 8, 5, "", "p2", (4, 1, 2, 64, 2, 0)),
    ("k5_str_64_16_8x8_b", "plain", 1031, 64, 16, 8, 8, 5, "", "p2", (4, 2, 2, 64, 2, 0)),
    ("k5_str_32_32_7x7_a", "plain", 3, 32, 32, 7, 7, 5, "", "p2", (4, 3, 2, 32, 2, 0)),
    ("k5_str_32_32_7x7_b", "plain", 2054, 32, 32, 7, 7, 5, "", "p2", (4, 4, 2, 32, 2, 0)),
    ("k5_str_16_40_5x13_a", "plain", 2, 16, 40, 5, 13, 5, "", "p3", (4, 2, 2, 16, 2, 0)),
    ("k5_str_16_40_5x13_b", "plain", 1543, 16, 40, 5, 13, 5, "", "p3", (4, 3, 2, 16, 2, 0)),
    ("k5_res_16_32_7x7_clipped", "plain", 3, 16, 32, 7, 7, 5, "", "p0", (1, 3, 0, 0, 0, 0)),
    ("k5_res_16_16_7x7_x_offset", "plain", 50, 16, 16, 7, 7, 5, "", "p0+xoff", (1, 6, 0, 0, 0, 0)),
    ("k5_str_ctx_16_64_7x7_y_offset", "ctx", 23, 16, 64, 7, 7, 5, "", "c0+yoff", (4, 5, 2, 16, 2, 1)),
    ("k5_str_32_64_7x7_xy_offset", "plain", 10, 32, 64, 7, 7, 5, "", "p2+xoff+yoff", (4, 3, 2, 32, 2, 0)),
    ("k5_refused_64_64_16x16", "plain", 3, 64, 64, 16, 16, 5, "", "p0", (0, 0, 0, 0, 0, 0)),
    ("k5_refused_ctx_64_16_16x16", "ctx", 3, 64, 16, 16, 16, 5, "", "c0", (0, 0, 0, 0, 0, 0)),
]


def cases():
    return [_case(r) for r in ROWS]


# ---- the weight gradient at ks = 5 (usf_conv_wgrad_k5_f32): (cin, cout, H, W) -> the instantiation (tiles per wave) at 256 units ---
# inputs / forms / the fp64 statement are tests/wide_wgrad_cases.py's.  Between them the rows launch every instantiation of
# usf_conv_wgrad_k5.hip; the tap-group count is 5 (one grid row per tap row) for every shape.
WGRAD_ROWS = [
    ((1, 1, 2, 2), 2), ((3, 5, 3, 5), 2), ((16, 16, 7, 7), 2), ((17, 33, 7, 7), 11), ((8, 16, 7, 7), 2), ((64, 64, 7, 7), 21),
    ((32, 32, 9, 9), 6), ((12, 16, 16, 16), 2), ((16, 32, 5, 5), 3), ((33, 64, 7, 7), 16),
    ((64, 32, 1, 112), 11),                      # the largest served LDS image: 163 832 of 163 840 bytes
]
# 300 rows: the grid is 103 blocks per tap row at 256 compute units (52 for the largest image), so blocks run three samples and two
WGRAD_BATCHES = (1, 5, 300)
WGRAD_REFUSED = [(65, 16, 7, 7, 5), (16, 65, 7, 7, 5), (16, 16, 1, 257, 5), (16, 16, 7, 7, 3), (16, 16, 7, 7, 7), (16, 16, 7, 7, 1),
                 (64, 64, 16, 16, 5)]           # the last: 169 400 bytes of LDS image


def wgrad_tiles_per_wave(cin, cout):
    """tap row 0 holds COT * (CIT * 5 + 1) tiles over four waves, rounded up to an instantiation"""
    need = -(-((cout + 15) // 16 * ((cin + 15) // 16 * 5 + 1)) // 4)
    return next(n for n in (2, 3, 6, 11, 16, 21) if need <= n)


# ---- the context column's gradient at ks = 5 (usf_conv_ctx_wgrad_f32) ---------------------------------------------------------------
CTX_WGRAD_ROWS = [(cout, H, W, stride, B) for cout in (7, 32) for H, W in ((1, 1), (2, 3), (7, 7)) for stride in (0, 1) for B in (1, 33)]
