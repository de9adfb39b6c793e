"""The "same" convolution at ks = 4, launch by launch: the case tables of tests/test_conv4_cpu.py and
tests/test_conv4_kernels_gpu.py.  Importable without a GPU and without the library.  The case builder, the data, the plane
layout, the guarded buffer and the checker are tests/conv_kernel_cases.py's; the fp64 / fp32 STATEMENTS are this file's own: an
even kernel is not symmetric, and the shared statement pads ks // 2 on both sides.

Placement.  nn.Conv2d(..., 4, padding="same") puts ONE zero before and TWO after the image in each axis,
    y[p] = sum_t w[t] x[p + t - 1]            F.conv2d(F.pad(x, (1, 2, 1, 2)), w)
(usf_conv2d_same_f32 / _ctx_f32 at ks = 4).  Its data gradient is the MIRRORED placement on the flipped, transposed weight,
    y[p] = sum_t w[t] x[p + t - 2]            F.conv2d(F.pad(x, (2, 1, 2, 1)), w)
(usf_conv2d_same_pad_f32 with pad_before = 2).  Every row exists in both placements: the twin of a row carries "+mir" in its
options and "_m" behind its name.  The mirrored entry point takes usf_conv2d_same_f32's arguments and has no context form, so
the twin of a ctx row is the plain call on the same shape (preset c0 -> p0, c1 -> p1).

A row has the format of conv_kernel_cases.ROWS: (name, entry, B, cin, cout, H, W, ks, knobs, opts, expect),
  expect  (kernel, S, NB, CP, NCT, CTX) from usf_conv2d_same_variant at 256 compute units: kernel 1 = weights resident in the LDS,
          kernel 4 = weights streamed (NB = 32-value k-blocks per slab, CP = padded input channels, NCT = slabs in the ring),
          kernel 0 = refused with -3, nothing launched.  The probe has one answer for both placements (the padded image is
          (H + 3) x (W + 3) either way); whichever kernel the library gives a shape, the table records it.
Rows named *_a / *_b are the two batches of one shape, as in tests/conv5_cases.py: (a) one sample fewer than fit a group, so S
is clipped to the batch (B = 1 where one sample fits); (b) B = S (2 * 256 + k) + r, 0 < r < S: blocks run three groups and two,
the last group is ragged, the streamed kernel's ring is carried across groups.  (a)'s outputs are a bit-exact prefix of (b)'s.

K = 16 cp with cp a multiple of 8 is a multiple of 128: a whole number of 32-blocks and of 64-value slabs.  The 5 x 5 table's
"short last slab" and "K padded beyond the taps" regimes cannot occur at ks = 4 and are not faked here.
"""
import torch
import torch.nn.functional as F

from conv_kernel_cases import _case as _base_case, _leaky, LEAKY, NONE, MARGIN  # noqa: F401

# max over this table (both placements) of |fp32 statement - fp64 statement| / (U * A), measured on a CPU
# (tests/test_conv4_cpu.py prints it per entry), rounded up in the second digit.  The CPU test asserts that the fp32 statement
# stays inside it; the device is held to MARGIN * K32_4 * U * A per element.  It comes from the fp32 CPU statement, never from a
# kernel.  Measured: 8.238 (k4_ctx_16_64_7x7_b_m; torch's placement plain 5.267, ctx 6.094; mirrored 8.238 -- F.conv2d's fp32
# sums run in the CPU library's order, which is further from fp64 than the tap-by-tap statement behind K32_5).
K32_4 = 8.3

# (tag, entry, cin, cout, H, W, opts, k): the shapes with two batches each
FAMILIES = [
    ("1_7_1x1", "plain", 1, 7, 1, 1, "p0", 1),                   # only tap (1, 1) reads inside ((2, 2) in the mirrored placement)
    ("ctx_5_16_2x3", "ctx", 5, 16, 2, 3, "c0", 2),               # smaller than the kernel in both axes, not square; cp = 8
    ("16_16_7x7", "plain", 16, 16, 7, 7, "p1", 3),
    ("ctx_16_40_7x7", "ctx", 16, 40, 7, 7, "c1", 1),
    ("5_64_8x8", "plain", 5, 64, 8, 8, "p2", 2),
    ("64_64_7x7", "plain", 64, 64, 7, 7, "p3", 1),               # the budget case: two samples beside the ring
    ("ctx_64_64_7x7", "ctx", 64, 64, 7, 7, "c1", 2),
    ("64_64_8x8", "plain", 64, 64, 8, 8, "p0", 1),
    ("ctx_64_64_8x8", "ctx", 64, 64, 8, 8, "c0", 3),
    ("ctx_16_64_7x7", "ctx", 16, 64, 7, 7, "c0", 3),
    ("33_64_16x16", "plain", 33, 64, 16, 16, "p1", 1),           # cp = 40
    ("ctx_33_64_16x16", "ctx", 33, 64, 16, 16, "c1", 2),         # (the streamed kernel's four-tile context instantiation)
    ("ctx_64_7_7x7", "ctx", 64, 7, 7, 7, "c1", 2),               # one tile of output channels
    ("64_16_8x8", "plain", 64, 16, 8, 8, "p2", 3),               # one tile of output channels, one row tile per wave
    ("ctx_64_16_8x8", "ctx", 64, 16, 8, 8, "c0", 1),
    ("32_32_7x7", "plain", 32, 32, 7, 7, "p2", 1),
    ("16_40_5x13", "plain", 16, 40, 5, 13, "p3", 2),             # three tiles of output channels
]
_MIRROR_PRESET = {"c0": "p0", "c1": "p1"}


def _twin(entry, opts):
    """the mirrored twin's (entry, opts) of a row"""
    o = opts.split("+")
    return "plain", "+".join([_MIRROR_PRESET.get(o[0], o[0])] + o[1:] + ["mir"])


def generate_rows(probe):
    """probe(entry, B, cin, cout, H, W, ks, aligned, knobs) -> the answer dict of usf_conv2d_same_variant at 256 compute units"""
    rows = []

    def add1(name, entry, B, cin, cout, H, W, opts):
        aligned = not ("xoff" in opts or "yoff" in opts)
        a = probe(entry, B, cin, cout, H, W, 4, aligned, "")
        exp = (a["kernel"], a["S"], a["NB"], a["CP"], a["NCT"], a["CTX"]) if a["kernel"] else (0, 0, 0, 0, 0, 0)
        rows.append((name, entry, B, cin, cout, H, W, 4, "", opts, exp))

    def add(name, entry, B, cin, cout, H, W, opts):
        add1(name, entry, B, cin, cout, H, W, opts)
        t_entry, t_opts = _twin(entry, opts)
        add1(name + "_m", t_entry, B, cin, cout, H, W, t_opts)

    for tag, entry, cin, cout, H, W, opts, k in FAMILIES:
        best = probe(entry, 1 << 16, cin, cout, H, W, 4, True, "")["S"]
        add(f"k4_{tag}_a", entry, max(1, best - 1), cin, cout, H, W, opts)
        add(f"k4_{tag}_b", entry, best * (2 * 256 + k) + max(1, best // 2) if best > 1 else 2 * 256 + k, cin, cout, H, W, opts)
    add("k4_16_32_7x7_clipped", "plain", 3, 16, 32, 7, 7, "p0")
    add("k4_16_16_7x7_x_offset", "plain", 50, 16, 16, 7, 7, "p0+xoff")
    add("k4_ctx_16_64_7x7_y_offset", "ctx", 23, 16, 64, 7, 7, "c0+yoff")
    add("k4_64_64_7x7_xy_offset", "plain", 10, 64, 64, 7, 7, "p2+xoff+yoff")
    # no plan holds 64 input channels of a 16 x 16 map (19 x 19 positions x 3 planes x 144 B = 155 952 B beside a ring or the planes)
    add("k4_refused_64_64_16x16", "plain", 3, 64, 64, 16, 16, "p0")
    add("k4_refused_ctx_64_16_16x16", "ctx", 3, 64, 16, 16, 16, "c0")
    return rows


# ---- the table (generate_rows with the library's answers; tests/test_conv4_cpu.py holds the two equal) -------------------------
ROWS = [
    ("k4_1_7_1x1_a", "plain", 7, 1, 7, 1, 1, 4, "", "p0", (1, 7, 0, 0, 0, 0)),
    ("k4_1_7_1x1_a_m", "plain", 7, 1, 7, 1, 1, 4, "", "p0+mir", (1, 7, 0, 0, 0, 0)),
    ("k4_1_7_1x1_b", "plain", 4108, 1, 7, 1, 1, 4, "", "p0", (1, 8, 0, 0, 0, 0)),
    ("k4_1_7_1x1_b_m", "plain", 4108, 1, 7, 1, 1, 4, "", "p0+mir", (1, 8, 0, 0, 0, 0)),
    ("k4_ctx_5_16_2x3_a", "ctx", 7, 5, 16, 2, 3, 4, "", "c0", (1, 7, 0, 0, 0, 1)),
    ("k4_ctx_5_16_2x3_a_m", "plain", 7, 5, 16, 2, 3, 4, "", "p0+mir", (1, 7, 0, 0, 0, 0)),
    ("k4_ctx_5_16_2x3_b", "ctx", 4116, 5, 16, 2, 3, 4, "", "c0", (1, 8, 0, 0, 0, 1)),
    ("k4_ctx_5_16_2x3_b_m", "plain", 4116, 5, 16, 2, 3, 4, "", "p0+mir", (1, 8, 0, 0, 0, 0)),
    ("k4_16_16_7x7_a", "plain", 7, 16, 16, 7, 7, 4, "", "p1", (1, 7, 0, 0, 0, 0)),
    ("k4_16_16_7x7_a_m", "plain", 7, 16, 16, 7, 7, 4, "", "p1+mir", (1, 7, 0, 0, 0, 0)),
    ("k4_16_16_7x7_b", "plain", 4124, 16, 16, 7, 7, 4, "", "p1", (1, 8, 0, 0, 0, 0)),
    ("k4_16_16_7x7_b_m", "plain", 4124, 16, 16, 7, 7, 4, "", "p1+mir", (1, 8, 0, 0, 0, 0)),
    ("k4_ctx_16_40_7x7_a", "ctx", 4, 16, 40, 7, 7, 4, "", "c1", (1, 4, 0, 0, 0, 1)),
    ("k4_ctx_16_40_7x7_a_m", "plain", 4, 16, 40, 7, 7, 4, "", "p1+mir", (1, 4, 0, 0, 0, 0)),
    ("k4_ctx_16_40_7x7_b", "ctx", 2567, 16, 40, 7, 7, 4, "", "c1", (1, 5, 0, 0, 0, 1)),
    ("k4_ctx_16_40_7x7_b_m", "plain", 2567, 16, 40, 7, 7, 4, "", "p1+mir", (1, 5, 0, 0, 0, 0)),
    ("k4_5_64_8x8_a", "plain", 7, 5, 64, 8, 8, 4, "", "p2", (1, 7, 0, 0, 0, 0)),
    ("k4_5_64_8x8_a_m", "plain", 7, 5, 64, 8, 8, 4, "", "p2+mir", (1, 7, 0, 0, 0, 0)),
    ("k4_5_64_8x8_b", "plain", 4116, 5, 64, 8, 8, 4, "", "p2", (1, 8, 0, 0, 0, 0)),
    ("k4_5_64_8x8_b_m", "plain", 4116, 5, 64, 8, 8, 4, "", "p2+mir", (1, 8, 0, 0, 0, 0)),
    ("k4_64_64_7x7_a", "plain", 1, 64, 64, 7, 7, 4, "", "p3", (4, 1, 2, 64, 2, 0)),
    ("k4_64_64_7x7_a_m", "plain", 1, 64, 64, 7, 7, 4, "", "p3+mir", (4, 1, 2, 64, 2, 0)),
    ("k4_64_64_7x7_b", "plain", 1027, 64, 64, 7, 7, 4, "", "p3", (4, 2, 2, 64, 2, 0)),
    ("k4_64_64_7x7_b_m", "plain", 1027, 64, 64, 7, 7, 4, "", "p3+mir", (4, 2, 2, 64, 2, 0)),
    ("k4_ctx_64_64_7x7_a", "ctx", 1, 64, 64, 7, 7, 4, "", "c1", (4, 1, 2, 64, 2, 1)),
    ("k4_ctx_64_64_7x7_a_m", "plain", 1, 64, 64, 7, 7, 4, "", "p1+mir", (4, 1, 2, 64, 2, 0)),
    ("k4_ctx_64_64_7x7_b", "ctx", 1029, 64, 64, 7, 7, 4, "", "c1", (4, 2, 2, 64, 2, 1)),
    ("k4_ctx_64_64_7x7_b_m", "plain", 1029, 64, 64, 7, 7, 4, "", "p1+mir", (4, 2, 2, 64, 2, 0)),
    ("k4_64_64_8x8_a", "plain", 1, 64, 64, 8, 8, 4, "", "p0", (4, 1, 2, 64, 2, 0)),
    ("k4_64_64_8x8_a_m", "plain", 1, 64, 64, 8, 8, 4, "", "p0+mir", (4, 1, 2, 64, 2, 0)),
    ("k4_64_64_8x8_b", "plain", 1027, 64, 64, 8, 8, 4, "", "p0", (4, 2, 2, 64, 2, 0)),
    ("k4_64_64_8x8_b_m", "plain", 1027, 64, 64, 8, 8, 4, "", "p0+mir", (4, 2, 2, 64, 2, 0)),
    ("k4_ctx_64_64_8x8_a", "ctx", 1, 64, 64, 8, 8, 4, "", "c0", (4, 1, 2, 64, 2, 1)),
    ("k4_ctx_64_64_8x8_a_m", "plain", 1, 64, 64, 8, 8, 4, "", "p0+mir", (4, 1, 2, 64, 2, 0)),
    ("k4_ctx_64_64_8x8_b", "ctx", 1031, 64, 64, 8, 8, 4, "", "c0", (4, 2, 2, 64, 2, 1)),
    ("k4_ctx_64_64_8x8_b_m", "plain", 1031, 64, 64, 8, 8, 4, "", "p0+mir", (4, 2, 2, 64, 2, 0)),
    ("k4_ctx_16_64_7x7_a", "ctx", 3, 16, 64, 7, 7, 4, "", "c0", (1, 3, 0, 0, 0, 1)),
    ("k4_ctx_16_64_7x7_a_m", "plain", 3, 16, 64, 7, 7, 4, "", "p0+mir", (1, 3, 0, 0, 0, 0)),
    ("k4_ctx_16_64_7x7_b", "ctx", 2062, 16, 64, 7, 7, 4, "", "c0", (1, 4, 0, 0, 0, 1)),
    ("k4_ctx_16_64_7x7_b_m", "plain", 2062, 16, 64, 7, 7, 4, "", "p0+mir", (1, 4, 0, 0, 0, 0)),
    ("k4_33_64_16x16_a", "plain", 1, 33, 64, 16, 16, 4, "", "p1", (4, 1, 2, 40, 2, 0)),
    ("k4_33_64_16x16_a_m", "plain", 1, 33, 64, 16, 16, 4, "", "p1+mir", (4, 1, 2, 40, 2, 0)),
    ("k4_33_64_16x16_b", "plain", 513, 33, 64, 16, 16, 4, "", "p1", (4, 1, 2, 40, 2, 0)),
    ("k4_33_64_16x16_b_m", "plain", 513, 33, 64, 16, 16, 4, "", "p1+mir", (4, 1, 2, 40, 2, 0)),
    ("k4_ctx_33_64_16x16_a", "ctx", 1, 33, 64, 16, 16, 4, "", "c1", (4, 1, 2, 40, 2, 1)),
    ("k4_ctx_33_64_16x16_a_m", "plain", 1, 33, 64, 16, 16, 4, "", "p1+mir", (4, 1, 2, 40, 2, 0)),
    ("k4_ctx_33_64_16x16_b", "ctx", 514, 33, 64, 16, 16, 4, "", "c1", (4, 1, 2, 40, 2, 1)),
    ("k4_ctx_33_64_16x16_b_m", "plain", 514, 33, 64, 16, 16, 4, "", "p1+mir", (4, 1, 2, 40, 2, 0)),
    ("k4_ctx_64_7_7x7_a", "ctx", 2, 64, 7, 7, 7, 4, "", "c1", (4, 2, 2, 64, 2, 1)),
    ("k4_ctx_64_7_7x7_a_m", "plain", 2, 64, 7, 7, 7, 4, "", "p1+mir", (4, 2, 2, 64, 2, 0)),
    ("k4_ctx_64_7_7x7_b", "ctx", 1543, 64, 7, 7, 7, 4, "", "c1", (4, 3, 2, 64, 2, 1)),
    ("k4_ctx_64_7_7x7_b_m", "plain", 1543, 64, 7, 7, 7, 4, "", "p1+mir", (4, 3, 2, 64, 2, 0)),
    ("k4_64_16_8x8_a", "plain", 1, 64, 16, 8, 8, 4, "", "p2", (4, 1, 2, 64, 2, 0)),
    ("k4_64_16_8x8_a_m", "plain", 1, 64, 16, 8, 8, 4, "", "p2+mir", (4, 1, 2, 64, 2, 0)),
    ("k4_64_16_8x8_b", "plain", 1031, 64, 16, 8, 8, 4, "", "p2", (4, 2, 2, 64, 2, 0)),
    ("k4_64_16_8x8_b_m", "plain", 1031, 64, 16, 8, 8, 4, "", "p2+mir", (4, 2, 2, 64, 2, 0)),
    ("k4_ctx_64_16_8x8_a", "ctx", 1, 64, 16, 8, 8, 4, "", "c0", (4, 1, 2, 64, 2, 1)),
    ("k4_ctx_64_16_8x8_a_m", "plain", 1, 64, 16, 8, 8, 4, "", "p0+mir", (4, 1, 2, 64, 2, 0)),
    ("k4_ctx_64_16_8x8_b", "ctx", 1027, 64, 16, 8, 8, 4, "", "c0", (4, 2, 2, 64, 2, 1)),
    ("k4_ctx_64_16_8x8_b_m", "plain", 1027, 64, 16, 8, 8, 4, "", "p0+mir", (4, 2, 2, 64, 2, 0)),
    ("k4_32_32_7x7_a", "plain", 1, 32, 32, 7, 7, 4, "", "p2", (1, 1, 0, 0, 0, 0)),
    ("k4_32_32_7x7_a_m", "plain", 1, 32, 32, 7, 7, 4, "", "p2+mir", (1, 1, 0, 0, 0, 0)),
    ("k4_32_32_7x7_b", "plain", 1027, 32, 32, 7, 7, 4, "", "p2", (1, 2, 0, 0, 0, 0)),
    ("k4_32_32_7x7_b_m", "plain", 1027, 32, 32, 7, 7, 4, "", "p2+mir", (1, 2, 0, 0, 0, 0)),
    ("k4_16_40_5x13_a", "plain", 3, 16, 40, 5, 13, 4, "", "p3", (1, 3, 0, 0, 0, 0)),
    ("k4_16_40_5x13_a_m", "plain", 3, 16, 40, 5, 13, 4, "", "p3+mir", (1, 3, 0, 0, 0, 0)),
    ("k4_16_40_5x13_b", "plain", 2058, 16, 40, 5, 13, 4, "", "p3", (1, 4, 0, 0, 0, 0)),
    ("k4_16_40_5x13_b_m", "plain", 2058, 16, 40, 5, 13, 4, "", "p3+mir", (1, 4, 0, 0, 0, 0)),
    ("k4_16_32_7x7_clipped", "plain", 3, 16, 32, 7, 7, 4, "", "p0", (1, 3, 0, 0, 0, 0)),
    ("k4_16_32_7x7_clipped_m", "plain", 3, 16, 32, 7, 7, 4, "", "p0+mir", (1, 3, 0, 0, 0, 0)),
    ("k4_16_16_7x7_x_offset", "plain", 50, 16, 16, 7, 7, 4, "", "p0+xoff", (1, 8, 0, 0, 0, 0)),
    ("k4_16_16_7x7_x_offset_m", "plain", 50, 16, 16, 7, 7, 4, "", "p0+xoff+mir", (1, 8, 0, 0, 0, 0)),
    ("k4_ctx_16_64_7x7_y_offset", "ctx", 23, 16, 64, 7, 7, 4, "", "c0+yoff", (1, 4, 0, 0, 0, 1)),
    ("k4_ctx_16_64_7x7_y_offset_m", "plain", 23, 16, 64, 7, 7, 4, "", "p0+yoff+mir", (1, 4, 0, 0, 0, 0)),
    ("k4_64_64_7x7_xy_offset", "plain", 10, 64, 64, 7, 7, 4, "", "p2+xoff+yoff", (4, 2, 2, 64, 2, 0)),
    ("k4_64_64_7x7_xy_offset_m", "plain", 10, 64, 64, 7, 7, 4, "", "p2+xoff+yoff+mir", (4, 2, 2, 64, 2, 0)),
    ("k4_refused_64_64_16x16", "plain", 3, 64, 64, 16, 16, 4, "", "p0", (0, 0, 0, 0, 0, 0)),
    ("k4_refused_64_64_16x16_m", "plain", 3, 64, 64, 16, 16, 4, "", "p0+mir", (0, 0, 0, 0, 0, 0)),
    ("k4_refused_ctx_64_16_16x16", "ctx", 3, 64, 16, 16, 16, 4, "", "c0", (0, 0, 0, 0, 0, 0)),
    ("k4_refused_ctx_64_16_16x16_m", "plain", 3, 64, 16, 16, 16, 4, "", "p0+mir", (0, 0, 0, 0, 0, 0)),
]


def _case(row):
    c = _base_case(row)
    c.mirror = "mir" in row[9].split("+")
    c.pad_before = 2 if c.mirror else 1
    return c


def cases():
    return [_case(r) for r in ROWS]


def family(c):
    return (c.entry, c.cin, c.cout, c.H, c.W, c.ks, c.preset, c.xoff, c.yoff, c.mirror)


# ---- the statements ---------------------------------------------------------------------------------------------------------------
def conv4(a, w, pad_before):
    """the 4 x 4 "same" convolution with pad_before zeros before and 3 - pad_before after the image in each axis"""
    pb, pa = pad_before, 3 - pad_before
    return F.conv2d(F.pad(a, (pb, pa, pb, pa)), w)


def forward(c, d, dtype):
    """(y, A) in `dtype` on d's device: the entry point's formula and the same formula with every term replaced by its magnitude
    (conv_kernel_cases.forward for the plain and ctx entries, with this file's placement)"""
    t = lambda v: None if v is None else v.to(dtype)
    x, w, bias = t(d.x), t(d.w), t(d.bias)
    a = _leaky(x, c.get("in_act", NONE), c.get("in_slope", 0.0))
    if d.in_mul is not None:
        a = a * t(d.in_mul)
    y = conv4(a, w, c.pad_before)
    A = conv4(a.abs(), w.abs(), c.pad_before)
    if bias is not None:
        y = y + bias.view(1, -1, 1, 1)
        A = A + bias.abs().view(1, -1, 1, 1)
    if c.entry == "ctx":
        assert not c.mirror
        ones = torch.ones(1, 1, c.H, c.W, dtype=dtype, device=x.device)
        wc = t(d.w_ctx).view(c.cout, 1, 4, 4)
        cx = t(d.ctx if c.ctx_stride else d.ctx[:1].expand(c.B)).view(-1, 1, 1, 1)
        y = y + cx * conv4(ones, wc, 1)
        A = A + cx.abs() * conv4(ones, wc.abs(), 1)
    return _leaky(y, c.out_act, c.out_slope), A


def reference(c, d):
    """(ref64, A64)"""
    return forward(c, d, torch.float64)


# ---- the weight gradient at ks = 4 (usf_conv_wgrad_k4_f32): (cin, cout, H, W) -> the instantiation (tiles per wave) at 256 units ---
# inputs / forms are tests/wide_wgrad_cases.py's; the fp64 statement is wgrad_ref64 below (explicit F.pad).  Between them the rows
# launch every instantiation the kernel-4 plan uses (all six); the tap-group count is 4 (one grid row per tap row).
WGRAD_ROWS = [
    ((1, 1, 2, 2), 2), ((3, 5, 3, 5), 2), ((16, 16, 7, 7), 2), ((17, 33, 7, 7), 11), ((8, 16, 7, 7), 2), ((64, 64, 7, 7), 21),
    ((32, 32, 9, 9), 6), ((12, 16, 16, 16), 2), ((16, 32, 5, 5), 3), ((33, 64, 7, 7), 16),
    ((64, 32, 1, 112), 11),                      # the largest served LDS image: 163 832 of 163 840 bytes (the 5 x 5 geometry)
]
WGRAD_BATCHES = (1, 5, 300)
WGRAD_REFUSED = [(65, 16, 7, 7, 4), (16, 65, 7, 7, 4), (16, 16, 1, 257, 4), (16, 16, 7, 7, 1), (16, 16, 7, 7, 3), (16, 16, 7, 7, 5),
                 (16, 16, 7, 7, 6), (64, 64, 16, 16, 4)]           # the last: 169 400 bytes of LDS image


def wgrad_tiles_per_wave(cin, cout):
    """tap row 0 holds COT * (CIT * 4 + 1) tiles over four waves, rounded up to an instantiation"""
    need = -(-((cout + 15) // 16 * ((cin + 15) // 16 * 4 + 1)) // 4)
    return next(n for n in (2, 3, 6, 11, 16, 21) if need <= n)


def wgrad_ref64(x, dy, kw):
    """dW [cout, cin, 4, 4], db [cout] in fp64 in torch's placement: dW[co, ci, ty, tx] = sum dy[b, co, p] xin[b, ci, p + (ty - 1, tx - 1)]"""
    from wide_wgrad_cases import xin64
    v = F.pad(xin64(x, kw), (1, 2, 1, 2))
    B, cin = v.shape[:2]
    H, W = x.shape[2:]
    cols = F.unfold(v, 4).view(B, cin, 16, H * W)
    dW = torch.einsum("bop,bctp->oct", dy.double().flatten(2), cols).view(dy.shape[1], cin, 4, 4)
    return dW, dy.double().sum((0, 2, 3))


# ---- the context column's gradient at ks = 4 (usf_conv_ctx_wgrad_f32) ---------------------------------------------------------------
CTX_WGRAD_ROWS = [(cout, H, W, stride, B) for cout in (7, 32) for H, W in ((1, 1), (2, 3), (7, 7)) for stride in (0, 1) for B in (1, 33)]
