"""The "same" convolution's three kernels, launch by launch: the case table, a builder that knows only the header's contract
(include/usflows_hip.h, usflows_hip_internal.h), an fp64 and an fp32 statement of every form and a checker.  Importable
without a GPU and without the library; tests/test_conv_kernels_cpu.py proves the table's coverage from the probe's answers
(usf_conv2d_same_variant), tests/test_conv_kernels_gpu.py launches every row.

A row: (name, entry, B, cin, cout, H, W, ks, knobs, opts, expect)
  entry   plain / ctx / res / gate_mul / gate_add / gated (gated: cout = C, the GatedConv's channels; 2 C rows are packed)
  knobs   tuning knobs in force for the launch ("conv_wsp=0": the register-weight kernel, "conv_wreg=0": the first kernel)
  opts    option preset of the entry (OPTS) plus "xoff" / "yoff": that tensor starts one float behind a 16-byte boundary
  expect  (kernel, S, NB, CP, NCT, CTX) at 256 compute units; NB = CP = NCT = 0 for kernel 1; kernel 0: refused, nothing is
          launched -- return code 1 from the fused forms (the caller runs two passes), -3 from a plain / ctx call no kernel serves
Rows named *_a / *_b are the two batches of one shape: (a) small enough that the smallest-servable-S rule applies (or that S is
clipped), (b) B = S_best (2 * 256 + k) + r, 0 < r < S_best: some blocks run three groups, the others two, the last group is
ragged.  Both batches draw the same samples (numpy's generator fills sequentially), so (a)'s outputs must be a prefix of (b)'s.
"""
import numpy as np
import torch
import torch.nn.functional as F

U = 2.0 ** -24
MARGIN = 4.0                       # bf16x3 against fp32: other summation order, three of nine partial products dropped
# max over the table of |fp32 statement - fp64 statement| / (U * A), measured on a CPU: 5.002 (wsp_gadd_48_48_1x1; per entry
# plain 3.80, ctx 2.70, res 2.83, gate_mul 2.73, gate_add 5.00, gated 1.15), rounded up in the second digit.
# tests/test_conv_kernels_cpu.py asserts that the fp32 statement stays inside it; the device is held to MARGIN * K32 * U * A
# per element
K32 = 5.1
GUARD = 64                         # sentinel floats in front of and behind y
SENTINEL_BITS = 0x65A5A5A5         # 9.78e22: no result of the table comes near it


# the library's default of every tuning knob the case tables set (tests/test_image_grad_kernels_cpu.py holds them to the sources)
KNOB_DEFAULTS = {"conv_wsp": 1, "conv_wreg": 1, "conv_small_s": 1, "conv_wgrad_rsplit": 1, "conv_wgrad_blocks": 0}


class knobs:
    """library tuning knobs for the duration of a block; the previous values afterwards (a knob nobody has set reads as its default)"""

    def __init__(self, lib, kv):
        self.lib, self.kv, self.old = lib, kv, {}

    def __enter__(self):
        for k, v in self.kv.items():
            self.old[k] = self.lib.usf_get_tuning(k.encode(), KNOB_DEFAULTS[k])
            assert self.lib.usf_set_tuning(k.encode(), int(v)) == 0, k

    def __exit__(self, *exc):
        for k, v in self.old.items():
            assert self.lib.usf_set_tuning(k.encode(), int(v)) == 0, k


def sentinel():
    return torch.tensor([SENTINEL_BITS], dtype=torch.int32).view(torch.float32).item()


LEAKY, NONE = 1, 0                 # USF_ACT_LEAKY_RELU / USF_ACT_NONE
# option presets: in_act / in_slope / out_act / out_slope, in_mul (None, "rand": a 0 / 1 mask, "chan": whole channels masked),
# bias, ctx_stride, res_sign, gate_slope, gate_mul
OPTS = {
    "p0": dict(in_act=LEAKY, in_slope=0.01, out_act=NONE, out_slope=0.0, in_mul=None, bias=True),
    "p1": dict(in_act=NONE, in_slope=0.0, out_act=LEAKY, out_slope=0.0, in_mul="chan", bias=False),
    "p2": dict(in_act=LEAKY, in_slope=0.0, out_act=LEAKY, out_slope=0.01, in_mul="rand", bias=True),
    "p3": dict(in_act=LEAKY, in_slope=1.0, out_act=LEAKY, out_slope=1.0, in_mul=None, bias=True),
    "c0": dict(in_act=LEAKY, in_slope=0.01, out_act=LEAKY, out_slope=0.01, in_mul="rand", bias=True, ctx_stride=1),
    "c1": dict(in_act=NONE, in_slope=0.0, out_act=NONE, out_slope=0.0, in_mul=None, bias=False, ctx_stride=0),
    "r0": dict(in_act=LEAKY, in_slope=0.01, in_mul="chan", bias=True, res_sign=1.0),
    "r1": dict(in_act=NONE, in_slope=0.0, in_mul=None, bias=False, res_sign=-1.0),
    "g0": dict(gate_slope=0.01, gate_mul=True),
    "g1": dict(gate_slope=0.0, gate_mul=False),
    "g2": dict(gate_slope=1.0, gate_mul=True),
    "a0": dict(gate_slope=0.01),
    "a1": dict(gate_slope=0.0),
    "a2": dict(gate_slope=1.0),
    "m0": dict(in_act=LEAKY, in_slope=0.01, bias=True),
    "m1": dict(in_act=NONE, in_slope=0.0, bias=False),
}
WSP0, WREG0 = "conv_wsp=0", "conv_wreg=0"

# ---- the table ------------------------------------------------------------------------------------------------------------
ROWS = [
    ("wsp_16_16_7x7_a", "plain", 16, 16, 16, 7, 7, 3, "", "p0", (3, 1, 5, 16, 1, 0)),
    ("wsp_16_16_7x7_b", "plain", 2567, 16, 16, 7, 7, 3, "", "p0", (3, 5, 5, 16, 1, 0)),
    ("wsp_ctx_16_16_7x7_a", "ctx", 16, 16, 16, 7, 7, 3, "", "c0", (3, 1, 5, 16, 1, 1)),
    ("wsp_ctx_16_16_7x7_b", "ctx", 2572, 16, 16, 7, 7, 3, "", "c0", (3, 5, 5, 16, 1, 1)),
    ("wsp_16_32_7x7_a", "plain", 16, 16, 32, 7, 7, 3, "", "p1", (3, 1, 5, 16, 2, 0)),
    ("wsp_16_32_7x7_b", "plain", 2572, 16, 32, 7, 7, 3, "", "p1", (3, 5, 5, 16, 2, 0)),
    ("wsp_ctx_16_32_7x7_a", "ctx", 16, 16, 32, 7, 7, 3, "", "c1", (3, 1, 5, 16, 2, 1)),
    ("wsp_ctx_16_32_7x7_b", "ctx", 2572, 16, 32, 7, 7, 3, "", "c1", (3, 5, 5, 16, 2, 1)),
    ("wsp_16_48_5x5_a", "plain", 22, 16, 48, 5, 5, 3, "", "p2", (3, 1, 5, 16, 4, 0)),
    ("wsp_16_48_5x5_b", "plain", 3608, 16, 48, 5, 5, 3, "", "p2", (3, 7, 5, 16, 4, 0)),
    ("wsp_ctx_16_48_5x5_a", "ctx", 22, 16, 48, 5, 5, 3, "", "c0", (3, 1, 5, 16, 4, 1)),
    ("wsp_ctx_16_48_5x5_b", "ctx", 3601, 16, 48, 5, 5, 3, "", "c0", (3, 7, 5, 16, 4, 1)),
    ("wsp_16_64_7x7_a", "plain", 13, 16, 64, 7, 7, 3, "", "p3", (3, 1, 5, 16, 4, 0)),
    ("wsp_16_64_7x7_b", "plain", 2054, 16, 64, 7, 7, 3, "", "p3", (3, 4, 5, 16, 4, 0)),
    ("wsp_ctx_16_64_7x7_a", "ctx", 13, 16, 64, 7, 7, 3, "", "c1", (3, 1, 5, 16, 4, 1)),
    ("wsp_ctx_16_64_7x7_b", "ctx", 2058, 16, 64, 7, 7, 3, "", "c1", (3, 4, 5, 16, 4, 1)),
    ("wsp_32_16_8x8_a", "plain", 13, 32, 16, 8, 8, 3, "", "p0", (3, 1, 9, 32, 1, 0)),
    ("wsp_32_16_8x8_b", "plain", 2058, 32, 16, 8, 8, 3, "", "p0", (3, 4, 9, 32, 1, 0)),
    ("wsp_ctx_32_16_8x8_a", "ctx", 13, 32, 16, 8, 8, 3, "", "c0", (3, 1, 9, 32, 1, 1)),
    ("wsp_ctx_32_16_8x8_b", "ctx", 2058, 32, 16, 8, 8, 3, "", "c0", (3, 4, 9, 32, 1, 1)),
    ("wsp_32_32_7x7_a", "plain", 16, 32, 32, 7, 7, 3, "", "p1", (3, 1, 9, 32, 2, 0)),
    ("wsp_32_32_7x7_b", "plain", 2577, 32, 32, 7, 7, 3, "", "p1", (3, 5, 9, 32, 2, 0)),
    ("wsp_ctx_32_32_7x7_a", "ctx", 16, 32, 32, 7, 7, 3, "", "c1", (3, 1, 9, 32, 2, 1)),
    ("wsp_ctx_32_32_7x7_b", "ctx", 2572, 32, 32, 7, 7, 3, "", "c1", (3, 5, 9, 32, 2, 1)),
    ("wsp_32_48_3x4_a", "plain", 49, 32, 48, 3, 4, 3, "", "p2", (3, 1, 9, 32, 4, 0)),
    ("wsp_32_48_3x4_b", "plain", 8216, 32, 48, 3, 4, 3, "", "p2", (3, 16, 9, 32, 4, 0)),
    ("wsp_ctx_32_48_3x4_a", "ctx", 49, 32, 48, 3, 4, 3, "", "c0", (3, 1, 9, 32, 4, 1)),
    ("wsp_ctx_32_48_3x4_b", "ctx", 8232, 32, 48, 3, 4, 3, "", "c0", (3, 16, 9, 32, 4, 1)),
    ("wsp_32_64_2x2_a", "plain", 49, 32, 64, 2, 2, 3, "", "p3", (3, 3, 9, 32, 4, 0)),
    ("wsp_32_64_2x2_b", "plain", 8232, 32, 64, 2, 2, 3, "", "p3", (3, 16, 9, 32, 4, 0)),
    ("wsp_ctx_32_64_2x2_a", "ctx", 49, 32, 64, 2, 2, 3, "", "c1", (3, 3, 9, 32, 4, 1)),
    ("wsp_ctx_32_64_2x2_b", "ctx", 8232, 32, 64, 2, 2, 3, "", "c1", (3, 16, 9, 32, 4, 1)),
    ("wsp_48_16_5x5_a", "plain", 16, 48, 16, 5, 5, 3, "", "p0", (3, 1, 14, 48, 1, 0)),
    ("wsp_48_16_5x5_b", "plain", 2577, 48, 16, 5, 5, 3, "", "p0", (3, 5, 14, 48, 1, 0)),
    ("wsp_ctx_48_16_5x5_a", "ctx", 16, 48, 16, 5, 5, 3, "", "c0", (3, 1, 14, 48, 1, 1)),
    ("wsp_ctx_48_16_5x5_b", "ctx", 2572, 48, 16, 5, 5, 3, "", "c0", (3, 5, 14, 48, 1, 1)),
    ("wsp_48_32_8x8_a", "plain", 7, 48, 32, 8, 8, 3, "", "p1", (3, 1, 14, 48, 2, 0)),
    ("wsp_48_32_8x8_b", "plain", 1027, 48, 32, 8, 8, 3, "", "p1", (3, 2, 14, 48, 2, 0)),
    ("wsp_ctx_48_32_8x8_a", "ctx", 7, 48, 32, 8, 8, 3, "", "c1", (3, 1, 14, 48, 2, 1)),
    ("wsp_ctx_48_32_8x8_b", "ctx", 1029, 48, 32, 8, 8, 3, "", "c1", (3, 2, 14, 48, 2, 1)),
    ("wsp_48_48_8x8_a", "plain", 7, 48, 48, 8, 8, 3, "", "p2", (3, 1, 14, 48, 4, 0)),
    ("wsp_48_48_8x8_b", "plain", 1029, 48, 48, 8, 8, 3, "", "p2", (3, 2, 14, 48, 4, 0)),
    ("wsp_ctx_48_48_8x8_a", "ctx", 7, 48, 48, 8, 8, 3, "", "c0", (3, 1, 14, 48, 4, 1)),
    ("wsp_ctx_48_48_8x8_b", "ctx", 1029, 48, 48, 8, 8, 3, "", "c0", (3, 2, 14, 48, 4, 1)),
    ("wsp_48_64_8x8_a", "plain", 7, 48, 64, 8, 8, 3, "", "p3", (3, 1, 14, 48, 4, 0)),
    ("wsp_48_64_8x8_b", "plain", 1031, 48, 64, 8, 8, 3, "", "p3", (3, 2, 14, 48, 4, 0)),
    ("wsp_ctx_48_64_8x8_a", "ctx", 7, 48, 64, 8, 8, 3, "", "c1", (3, 1, 14, 48, 4, 1)),
    ("wsp_ctx_48_64_8x8_b", "ctx", 1029, 48, 64, 8, 8, 3, "", "c1", (3, 2, 14, 48, 4, 1)),
    ("wsp_32_48_1x1_a", "plain", 5, 32, 48, 1, 1, 3, "", "p0", (3, 12, 9, 32, 4, 0)),
    ("wsp_ctx_16_48_1x1_a", "ctx", 3, 16, 48, 1, 1, 3, "", "c0", (3, 12, 5, 16, 4, 1)),
    ("wsp_32_64_1x1_a", "plain", 5, 32, 64, 1, 1, 3, "", "p0", (3, 12, 9, 32, 4, 0)),
    ("wsp_ctx_16_64_1x1_a", "ctx", 3, 16, 64, 1, 1, 3, "", "c0", (3, 12, 5, 16, 4, 1)),
    ("wsp_16_32_3x4_nonsquare", "plain", 77, 16, 32, 3, 4, 3, "", "p2", (3, 2, 5, 16, 2, 0)),
    ("wsp_ctx_48_64_4x3_nonsquare", "ctx", 61, 48, 64, 4, 3, 3, "", "c0", (3, 1, 14, 48, 4, 1)),
    ("wsp_16_32_8x1_one_wide", "plain", 70, 16, 32, 8, 1, 3, "", "p0", (3, 3, 5, 16, 2, 0)),
    ("wsp_ctx_32_16_5x1_one_wide", "ctx", 33, 32, 16, 5, 1, 3, "", "c0", (3, 5, 9, 32, 1, 1)),
    ("wsp_res_16_64_1x1", "res", 29, 16, 64, 1, 1, 3, "", "r0", (3, 12, 5, 16, 4, 0)),
    ("wsp_gadd_48_48_1x1", "gate_add", 6149, 48, 48, 1, 1, 3, "", "a0", (3, 16, 14, 48, 4, 0)),
    ("wreg_32_64_4x1_one_wide", "plain", 45, 32, 64, 4, 1, 3, WSP0, "p2", (2, 16, 9, 32, 4, 0)),
    ("wsp_res_16_64_7x7_a", "res", 7, 16, 64, 7, 7, 3, "", "r0", (3, 1, 5, 16, 4, 0)),
    ("wsp_res_16_64_7x7_b", "res", 1027, 16, 64, 7, 7, 3, "", "r0", (3, 2, 5, 16, 4, 0)),
    ("wsp_gmul_16_64_7x7_a", "gate_mul", 7, 16, 64, 7, 7, 3, "", "g0", (3, 1, 5, 16, 4, 0)),
    ("wsp_gmul_16_64_7x7_b", "gate_mul", 1029, 16, 64, 7, 7, 3, "", "g0", (3, 2, 5, 16, 4, 0)),
    ("wsp_gadd_16_64_7x7_a", "gate_add", 7, 16, 64, 7, 7, 3, "", "a0", (3, 1, 5, 16, 4, 0)),
    ("wsp_gadd_16_64_7x7_b", "gate_add", 1031, 16, 64, 7, 7, 3, "", "a0", (3, 2, 5, 16, 4, 0)),
    ("wsp_res_32_16_7x7_a", "res", 16, 32, 16, 7, 7, 3, "", "r1", (3, 1, 9, 32, 1, 0)),
    ("wsp_res_32_16_7x7_b", "res", 2567, 32, 16, 7, 7, 3, "", "r1", (3, 5, 9, 32, 1, 0)),
    ("wsp_gmul_32_16_7x7_a", "gate_mul", 16, 32, 16, 7, 7, 3, "", "g1", (3, 1, 9, 32, 1, 0)),
    ("wsp_gmul_32_16_7x7_b", "gate_mul", 2572, 32, 16, 7, 7, 3, "", "g1", (3, 5, 9, 32, 1, 0)),
    ("wsp_gadd_32_16_7x7_a", "gate_add", 16, 32, 16, 7, 7, 3, "", "a1", (3, 1, 9, 32, 1, 0)),
    ("wsp_gadd_32_16_7x7_b", "gate_add", 2577, 32, 16, 7, 7, 3, "", "a1", (3, 5, 9, 32, 1, 0)),
    ("wsp_res_48_48_8x8_a", "res", 7, 48, 48, 8, 8, 3, "", "r0", (3, 1, 14, 48, 4, 0)),
    ("wsp_res_48_48_8x8_b", "res", 1027, 48, 48, 8, 8, 3, "", "r0", (3, 2, 14, 48, 4, 0)),
    ("wsp_gmul_48_48_8x8_a", "gate_mul", 7, 48, 48, 8, 8, 3, "", "g2", (3, 1, 14, 48, 4, 0)),
    ("wsp_gmul_48_48_8x8_b", "gate_mul", 1029, 48, 48, 8, 8, 3, "", "g2", (3, 2, 14, 48, 4, 0)),
    ("wsp_gadd_48_48_8x8_a", "gate_add", 7, 48, 48, 8, 8, 3, "", "a2", (3, 1, 14, 48, 4, 0)),
    ("wsp_gadd_48_48_8x8_b", "gate_add", 1031, 48, 48, 8, 8, 3, "", "a2", (3, 2, 14, 48, 4, 0)),
    ("wsp_res_32_32_8x8_a", "res", 10, 32, 32, 8, 8, 3, "", "r1", (3, 1, 9, 32, 2, 0)),
    ("wsp_res_32_32_8x8_b", "res", 1540, 32, 32, 8, 8, 3, "", "r1", (3, 3, 9, 32, 2, 0)),
    ("wsp_gmul_32_32_8x8_a", "gate_mul", 10, 32, 32, 8, 8, 3, "", "g0", (3, 1, 9, 32, 2, 0)),
    ("wsp_gmul_32_32_8x8_b", "gate_mul", 1543, 32, 32, 8, 8, 3, "", "g0", (3, 3, 9, 32, 2, 0)),
    ("wsp_gadd_32_32_8x8_a", "gate_add", 10, 32, 32, 8, 8, 3, "", "a0", (3, 1, 9, 32, 2, 0)),
    ("wsp_gadd_32_32_8x8_b", "gate_add", 1546, 32, 32, 8, 8, 3, "", "a0", (3, 3, 9, 32, 2, 0)),
    ("wreg_16_16_7x7_a", "plain", 31, 16, 16, 7, 7, 3, WSP0, "p0", (2, 10, 5, 16, 1, 0)),
    ("wreg_16_16_7x7_b", "plain", 5135, 16, 16, 7, 7, 3, WSP0, "p0", (2, 10, 5, 16, 1, 0)),
    ("wreg_ctx_16_16_7x7_a", "ctx", 31, 16, 16, 7, 7, 3, WSP0, "c0", (2, 10, 5, 16, 1, 1)),
    ("wreg_ctx_16_16_7x7_b", "ctx", 5145, 16, 16, 7, 7, 3, WSP0, "c0", (2, 10, 5, 16, 1, 1)),
    ("wreg_16_32_7x7_a", "plain", 16, 16, 32, 7, 7, 3, WSP0, "p1", (2, 5, 5, 16, 2, 0)),
    ("wreg_16_32_7x7_b", "plain", 2567, 16, 32, 7, 7, 3, WSP0, "p1", (2, 5, 5, 16, 2, 0)),
    ("wreg_ctx_16_32_7x7_a", "ctx", 16, 16, 32, 7, 7, 3, WSP0, "c1", (2, 5, 5, 16, 2, 1)),
    ("wreg_ctx_16_32_7x7_b", "ctx", 2572, 16, 32, 7, 7, 3, WSP0, "c1", (2, 5, 5, 16, 2, 1)),
    ("wreg_16_64_5x5_a", "plain", 16, 16, 64, 5, 5, 3, WSP0, "p2", (2, 5, 5, 16, 4, 0)),
    ("wreg_16_64_5x5_b", "plain", 2567, 16, 64, 5, 5, 3, WSP0, "p2", (2, 5, 5, 16, 4, 0)),
    ("wreg_ctx_16_64_5x5_a", "ctx", 16, 16, 64, 5, 5, 3, WSP0, "c0", (2, 5, 5, 16, 4, 1)),
    ("wreg_ctx_16_64_5x5_b", "ctx", 2572, 16, 64, 5, 5, 3, WSP0, "c0", (2, 5, 5, 16, 4, 1)),
    ("wreg_32_16_8x8_a", "plain", 13, 32, 16, 8, 8, 3, WSP0, "p3", (2, 4, 9, 32, 1, 0)),
    ("wreg_32_16_8x8_b", "plain", 2054, 32, 16, 8, 8, 3, WSP0, "p3", (2, 4, 9, 32, 1, 0)),
    ("wreg_ctx_32_16_8x8_a", "ctx", 13, 32, 16, 8, 8, 3, WSP0, "c1", (2, 4, 9, 32, 1, 1)),
    ("wreg_ctx_32_16_8x8_b", "ctx", 2058, 32, 16, 8, 8, 3, WSP0, "c1", (2, 4, 9, 32, 1, 1)),
    ("wreg_32_32_7x7_a", "plain", 16, 32, 32, 7, 7, 3, WSP0, "p0", (2, 5, 9, 32, 2, 0)),
    ("wreg_32_32_7x7_b", "plain", 2567, 32, 32, 7, 7, 3, WSP0, "p0", (2, 5, 9, 32, 2, 0)),
    ("wreg_ctx_32_32_7x7_a", "ctx", 16, 32, 32, 7, 7, 3, WSP0, "c0", (2, 5, 9, 32, 2, 1)),
    ("wreg_ctx_32_32_7x7_b", "ctx", 2572, 32, 32, 7, 7, 3, WSP0, "c0", (2, 5, 9, 32, 2, 1)),
    ("wreg_32_64_2x2_a", "plain", 49, 32, 64, 2, 2, 3, WSP0, "p1", (2, 16, 9, 32, 4, 0)),
    ("wreg_32_64_2x2_b", "plain", 8216, 32, 64, 2, 2, 3, WSP0, "p1", (2, 16, 9, 32, 4, 0)),
    ("wreg_ctx_32_64_2x2_a", "ctx", 49, 32, 64, 2, 2, 3, WSP0, "c1", (2, 16, 9, 32, 4, 1)),
    ("wreg_ctx_32_64_2x2_b", "ctx", 8232, 32, 64, 2, 2, 3, WSP0, "c1", (2, 16, 9, 32, 4, 1)),
    ("wreg_res_16_16_7x7_a", "res", 31, 16, 16, 7, 7, 3, WSP0, "r0", (2, 10, 5, 16, 1, 0)),
    ("wreg_res_16_16_7x7_b", "res", 5135, 16, 16, 7, 7, 3, WSP0, "r0", (2, 10, 5, 16, 1, 0)),
    ("wreg_res_32_32_3x4_a", "res", 49, 32, 32, 3, 4, 3, WSP0, "r1", (2, 16, 9, 32, 2, 0)),
    ("wreg_res_32_32_3x4_b", "res", 8232, 32, 32, 3, 4, 3, WSP0, "r1", (2, 16, 9, 32, 2, 0)),
    ("wreg_gmul_32_16_7x7_a", "gate_mul", 16, 32, 16, 7, 7, 3, WSP0, "g0", (2, 5, 9, 32, 1, 0)),
    ("wreg_gmul_32_16_7x7_b", "gate_mul", 2567, 32, 16, 7, 7, 3, WSP0, "g0", (2, 5, 9, 32, 1, 0)),
    ("wreg_gmul_16_32_5x5_a", "gate_mul", 31, 16, 32, 5, 5, 3, WSP0, "g1", (2, 10, 5, 16, 2, 0)),
    ("wreg_gmul_16_32_5x5_b", "gate_mul", 5145, 16, 32, 5, 5, 3, WSP0, "g1", (2, 10, 5, 16, 2, 0)),
    ("wreg_res_16_64_7x7_a", "res", 7, 16, 64, 7, 7, 3, WSP0, "r1", (2, 2, 5, 16, 4, 0)),
    ("wreg_res_16_64_7x7_b", "res", 1031, 16, 64, 7, 7, 3, WSP0, "r1", (2, 2, 5, 16, 4, 0)),
    ("wreg_refuses_gadd_16_16_7x7", "gate_add", 40, 16, 16, 7, 7, 3, WSP0, "a0", (0, 0, 0, 0, 0, 0)),
    ("wreg_refuses_48_in", "res", 40, 48, 16, 7, 7, 3, WSP0, "r1", (0, 0, 0, 0, 0, 0)),
    ("first_ks1_16_32_7x7", "plain", 37, 16, 32, 7, 7, 1, "", "p0", (1, 8, 0, 0, 0, 0)),
    ("first_ks1_ctx_5_7_6x6", "ctx", 19, 5, 7, 6, 6, 1, "", "c0", (1, 8, 0, 0, 0, 1)),
    ("first_1_16_7x7", "ctx", 21, 1, 16, 7, 7, 3, "", "c0", (1, 8, 0, 0, 0, 1)),
    ("first_3_32_8x8", "plain", 9, 3, 32, 8, 8, 3, "", "p1", (1, 8, 0, 0, 0, 0)),
    ("first_5_5_6x6", "plain", 30, 5, 5, 6, 6, 3, "", "p2", (1, 8, 0, 0, 0, 0)),
    ("first_33_16_7x7", "ctx", 11, 33, 16, 7, 7, 3, "", "c1", (1, 6, 0, 0, 0, 1)),
    ("first_64_7_8x8", "plain", 13, 64, 7, 8, 8, 3, "", "p0", (1, 2, 0, 0, 0, 0)),
    ("first_16_32_14x14", "plain", 5, 16, 32, 14, 14, 3, "", "p1", (1, 3, 0, 0, 0, 0)),
    ("first_32_32_16x16", "ctx", 3, 32, 32, 16, 16, 3, "", "c0", (1, 1, 0, 0, 0, 1)),
    ("first_16_16_9x9", "plain", 17, 16, 16, 9, 9, 3, "", "p3", (1, 8, 0, 0, 0, 0)),
    ("first_8_64_16x16", "plain", 2, 8, 64, 16, 16, 3, "", "p0", (1, 2, 0, 0, 0, 0)),
    ("first_48_16_3x27", "ctx", 7, 48, 16, 3, 27, 3, "", "c1", (1, 2, 0, 0, 0, 1)),
    ("first_16_32_1x1", "plain", 9, 16, 32, 1, 1, 3, "", "p2", (1, 8, 0, 0, 0, 0)),
    ("first_32_16_1x1", "plain", 300, 32, 16, 1, 1, 3, "", "p3", (1, 8, 0, 0, 0, 0)),
    ("first_64_32_8x8", "ctx", 3, 64, 32, 8, 8, 3, "", "c0", (1, 1, 0, 0, 0, 1)),
    ("wsp_16_16_3x9", "plain", 17, 16, 16, 3, 9, 3, "", "p3", (3, 1, 5, 16, 1, 0)),
    ("wsp_ctx_16_16_3x3", "ctx", 23, 16, 16, 3, 3, 3, "", "c1", (3, 3, 5, 16, 1, 1)),
    ("first_16_32_7x7_x_offset", "plain", 50, 16, 32, 7, 7, 3, "", "p0+xoff", (1, 8, 0, 0, 0, 0)),
    ("first_16_32_7x7_y_offset", "plain", 50, 16, 32, 7, 7, 3, "", "p2+yoff", (1, 8, 0, 0, 0, 0)),
    ("first_ctx_48_32_8x8_x_offset", "ctx", 9, 48, 32, 8, 8, 3, "", "c0+xoff", (1, 2, 0, 0, 0, 1)),
    ("refused_48_64_8x8_x_offset", "plain", 9, 48, 64, 8, 8, 3, "", "p0+xoff", (0, 0, 0, 0, 0, 0)),
    ("refused_ctx_48_48_8x8_wreg0", "ctx", 9, 48, 48, 8, 8, 3, WREG0, "c0", (0, 0, 0, 0, 0, 0)),
    ("first_16_32_7x7_wreg0_multi", "plain", 4171, 16, 32, 7, 7, 3, WREG0, "p0", (1, 8, 0, 0, 0, 0)),
    ("first_48_32_8x8_wreg0_multi", "plain", 1031, 48, 32, 8, 8, 3, WREG0, "p2", (1, 2, 0, 0, 0, 0)),
    ("first_ctx_48_16_5x5_wreg0_multi", "ctx", 4117, 48, 16, 5, 5, 3, WREG0, "c0", (1, 5, 0, 0, 0, 1)),
    ("first_16_16_2x2_wreg0_ragged", "plain", 25, 16, 16, 2, 2, 3, WREG0, "p1", (1, 8, 0, 0, 0, 0)),
    ("first_16_32_4x4_wreg0_ragged", "plain", 25, 16, 32, 4, 4, 3, WREG0, "p2", (1, 8, 0, 0, 0, 0)),
    ("first_16_64_7x7_wreg0_ragged", "plain", 25, 16, 64, 7, 7, 3, WREG0, "p3", (1, 8, 0, 0, 0, 0)),
    ("first_32_16_5x5_wreg0_ragged", "ctx", 17, 32, 16, 5, 5, 3, WREG0, "c1", (1, 8, 0, 0, 0, 1)),
    ("first_16_16_7x7_clipped", "plain", 3, 16, 16, 7, 7, 3, WREG0, "p0", (1, 3, 0, 0, 0, 0)),
    ("gated_C6_6x6_k3_B17", "gated", 17, 6, 6, 6, 6, 3, "", "m0", (1, 8, 0, 0, 0, 0)),
    ("gated_C16_7x7_k3_B41", "gated", 41, 16, 16, 7, 7, 3, "", "m1", (1, 8, 0, 0, 0, 0)),
    ("gated_C20_7x7_k3_B9", "gated", 9, 20, 20, 7, 7, 3, "", "m0", (1, 6, 0, 0, 0, 0)),
    ("gated_C32_8x8_k3_B2054", "gated", 2054, 32, 32, 8, 8, 3, "", "m1", (1, 2, 0, 0, 0, 0)),
    ("gated_C16_2x2_k3_B3", "gated", 3, 16, 16, 2, 2, 3, "", "m0", (1, 3, 0, 0, 0, 0)),
    ("gated_C32_7x7_k1_B12", "gated", 12, 32, 32, 7, 7, 1, "", "m1", (1, 8, 0, 0, 0, 0)),
    ("gated_C6_3x3_k3_B2049", "gated", 2049, 6, 6, 3, 3, 3, "", "m0", (1, 8, 0, 0, 0, 0)),
]


class Case(dict):
    __getattr__ = dict.__getitem__
    __setattr__ = dict.__setitem__


def _case(row):
    name, entry, B, cin, cout, H, W, ks, knobs, opts, expect = row
    o = opts.split("+")
    c = Case(name=name, entry=entry, B=B, cin=cin, cout=cout, H=H, W=W, ks=ks, knobs=dict(kv.split("=") for kv in knobs.split(",") if kv),
             preset=o[0], xoff="xoff" in o, yoff="yoff" in o, expect=tuple(expect))
    c.knobs = {k: int(v) for k, v in c.knobs.items()}
    c.update(OPTS[o[0]])
    c.C = cout if entry == "gated" else 0
    c.rows = 2 * cout if entry == "gated" else cout             # rows of the nn.Conv2d weight
    c.cout_arg = 32 * ((cout + 15) // 16) if entry == "gated" else cout
    return c


def cases():
    return [_case(r) for r in ROWS]


def family(c):
    """what the two batches of one shape share: everything but B and the name"""
    return (c.entry, c.cin, c.cout, c.H, c.W, c.ks, tuple(sorted(c.knobs.items())), c.preset, c.xoff, c.yoff)


# ---- how the table was made: the rules, with the probe's answers (cus = 256) filling in S and the expectation -------------------
WSP_SHAPES = {  # (cin, cout) -> (H, W): every reachable (CP, NCT) of the wave-specialised kernel, over the shapes the issue names
    (16, 16): (7, 7), (16, 32): (7, 7), (16, 48): (5, 5), (16, 64): (7, 7), (32, 16): (8, 8), (32, 32): (7, 7), (32, 48): (3, 4),
    (32, 64): (2, 2), (48, 16): (5, 5), (48, 32): (8, 8), (48, 48): (8, 8), (48, 64): (8, 8)}


def generate_rows(probe):
    """probe(entry, B, cin, cout, H, W, ks, aligned, knobs) -> the answer dict of usf_conv2d_same_variant at 256 compute units"""
    rows = []

    def exp(entry, B, cin, cout, H, W, ks, knobs, aligned=True):
        packed = 32 * ((cout + 15) // 16) if entry == "gated" else cout
        a = probe(entry, B, cin, packed, H, W, ks, aligned, knobs)
        return (a["kernel"], a["S"], a["NB"], a["CP"], a["NCT"], a["CTX"]) if a["kernel"] else (0, 0, 0, 0, 0, 0)

    def add(name, entry, B, cin, cout, H, W, ks, knobs, opts):
        aligned = not ("xoff" in opts or "yoff" in opts)
        rows.append((name, entry, B, cin, cout, H, W, ks, knobs, opts, exp(entry, B, cin, cout, H, W, ks, knobs, aligned)))

    def two_batches(tag, entry, cin, cout, H, W, knobs, opts, k):
        best = probe(entry, 1 << 16, cin, cout, H, W, 3, True, knobs)["S"]
        add(f"{tag}_a", entry, max(1, min(100, 3 * best + 1)) if H * W > 1 else 5, cin, cout, H, W, 3, knobs, opts)
        add(f"{tag}_b", entry, best * (2 * 256 + k) + max(1, best // 2) if best > 1 else 2 * 256 + k, cin, cout, H, W, 3, knobs, opts)

    # wave-specialised kernel: every (CP, NCT, CTX), two batches each
    for i, ((cin, cout), (H, W)) in enumerate(sorted(WSP_SHAPES.items())):
        two_batches(f"wsp_{cin}_{cout}_{H}x{W}", "plain", cin, cout, H, W, "", f"p{i % 4}", 1 + i % 3)
        two_batches(f"wsp_ctx_{cin}_{cout}_{H}x{W}", "ctx", cin, cout, H, W, "", f"c{i % 2}", 2)
    for cout in (48, 64):                                           # 1 x 1 pictures: S = 16 / 12 exceeds a small batch
        add(f"wsp_32_{cout}_1x1_a", "plain", 5, 32, cout, 1, 1, 3, "", "p0")
        add(f"wsp_ctx_16_{cout}_1x1_a", "ctx", 3, 16, cout, 1, 1, 3, "", "c0")
    add("wsp_16_32_3x4_nonsquare", "plain", 77, 16, 32, 3, 4, 3, "", "p2")
    add("wsp_ctx_48_64_4x3_nonsquare", "ctx", 61, 48, 64, 4, 3, 3, "", "c0")
    # pictures of one pixel and of one pixel's width: the divisors H W = 1 and W = 1 have no 32-bit magic number (cw_div)
    add("wsp_16_32_8x1_one_wide", "plain", 70, 16, 32, 8, 1, 3, "", "p0")
    add("wsp_ctx_32_16_5x1_one_wide", "ctx", 33, 32, 16, 5, 1, 3, "", "c0")
    add("wsp_res_16_64_1x1", "res", 29, 16, 64, 1, 1, 3, "", "r0")
    add("wsp_gadd_48_48_1x1", "gate_add", 2 * 256 * 12 + 5, 48, 48, 1, 1, 3, "", "a0")
    add("wreg_32_64_4x1_one_wide", "plain", 45, 32, 64, 4, 1, 3, WSP0, "p2")
    # the fused forms on it (16 -> 64 at 7 x 7: the residual lowers S from 4 to 2)
    for i, (cin, cout, H, W) in enumerate([(16, 64, 7, 7), (32, 16, 7, 7), (48, 48, 8, 8), (32, 32, 8, 8)]):
        two_batches(f"wsp_res_{cin}_{cout}_{H}x{W}", "res", cin, cout, H, W, "", f"r{i % 2}", 1)
        two_batches(f"wsp_gmul_{cin}_{cout}_{H}x{W}", "gate_mul", cin, cout, H, W, "", f"g{i % 3}", 2)
        two_batches(f"wsp_gadd_{cin}_{cout}_{H}x{W}", "gate_add", cin, cout, H, W, "", f"a{i % 3}", 3)
    # register-weight kernel (conv_wsp=0): all 12 instantiations, the forms it accepts, its documented refusals
    for i, (cin, cout, H, W) in enumerate([(16, 16, 7, 7), (16, 32, 7, 7), (16, 64, 5, 5), (32, 16, 8, 8), (32, 32, 7, 7), (32, 64, 2, 2)]):
        two_batches(f"wreg_{cin}_{cout}_{H}x{W}", "plain", cin, cout, H, W, WSP0, f"p{i % 4}", 1)
        two_batches(f"wreg_ctx_{cin}_{cout}_{H}x{W}", "ctx", cin, cout, H, W, WSP0, f"c{i % 2}", 2)
    two_batches("wreg_res_16_16_7x7", "res", 16, 16, 7, 7, WSP0, "r0", 1)
    two_batches("wreg_res_32_32_3x4", "res", 32, 32, 3, 4, WSP0, "r1", 2)
    two_batches("wreg_gmul_32_16_7x7", "gate_mul", 32, 16, 7, 7, WSP0, "g0", 1)
    two_batches("wreg_gmul_16_32_5x5", "gate_mul", 16, 32, 5, 5, WSP0, "g1", 2)
    two_batches("wreg_res_16_64_7x7", "res", 16, 64, 7, 7, WSP0, "r1", 3)   # (the largest residual group it stages: 2 * 64 * 49 floats)
    add("wreg_refuses_gadd_16_16_7x7", "gate_add", 40, 16, 16, 7, 7, 3, WSP0, "a0")
    add("wreg_refuses_48_in", "res", 40, 48, 16, 7, 7, 3, WSP0, "r1")
    # first kernel
    add("first_ks1_16_32_7x7", "plain", 37, 16, 32, 7, 7, 1, "", "p0")
    add("first_ks1_ctx_5_7_6x6", "ctx", 19, 5, 7, 6, 6, 1, "", "c0")
    for i, (cin, cout, H, W, B) in enumerate([(1, 16, 7, 7, 21), (3, 32, 8, 8, 9), (5, 5, 6, 6, 30), (33, 16, 7, 7, 11), (64, 7, 8, 8, 13),
                                              (16, 32, 14, 14, 5), (32, 32, 16, 16, 3), (16, 16, 9, 9, 17), (8, 64, 16, 16, 2),
                                              (48, 16, 3, 27, 7), (16, 32, 1, 1, 9), (32, 16, 1, 1, 300), (64, 32, 8, 8, 3)]):
        add(f"first_{cin}_{cout}_{H}x{W}", "plain" if i % 3 else "ctx", B, cin, cout, H, W, 3, "", f"p{i % 4}" if i % 3 else f"c{i % 2}")
    add("wsp_16_16_3x9", "plain", 17, 16, 16, 3, 9, 3, "", "p3")
    add("wsp_ctx_16_16_3x3", "ctx", 23, 16, 16, 3, 3, 3, "", "c1")
    add("first_16_32_7x7_x_offset", "plain", 50, 16, 32, 7, 7, 3, "", "p0+xoff")
    add("first_16_32_7x7_y_offset", "plain", 50, 16, 32, 7, 7, 3, "", "p2+yoff")
    add("first_ctx_48_32_8x8_x_offset", "ctx", 9, 48, 32, 8, 8, 3, "", "c0+xoff")
    # 48 -> 48 / 64 at 8 x 8 has no first-kernel form (its weight image alone is 131 / 175 KB of LDS): an unaligned tensor
    # or conv_wreg=0 is REFUSED there with -3, nothing is launched
    add("refused_48_64_8x8_x_offset", "plain", 9, 48, 64, 8, 8, 3, "", "p0+xoff")
    add("refused_ctx_48_48_8x8_wreg0", "ctx", 9, 48, 48, 8, 8, 3, WREG0, "c0")
    # the wave-specialised shapes under conv_wreg=0: more than one group per block, ragged last groups, all four patch shapes
    add("first_16_32_7x7_wreg0_multi", "plain", 8 * 2 * 256 + 8 * 9 + 3, 16, 32, 7, 7, 3, WREG0, "p0")
    add("first_48_32_8x8_wreg0_multi", "plain", 2 * (2 * 256 + 3) + 1, 48, 32, 8, 8, 3, WREG0, "p2")
    add("first_ctx_48_16_5x5_wreg0_multi", "ctx", 8 * (2 * 256 + 2) + 5, 48, 16, 5, 5, 3, WREG0, "c0")
    add("first_16_16_2x2_wreg0_ragged", "plain", 8 * 3 + 1, 16, 16, 2, 2, 3, WREG0, "p1")       # 16 x 16 full and last
    add("first_16_32_4x4_wreg0_ragged", "plain", 8 * 3 + 1, 16, 32, 4, 4, 3, WREG0, "p2")       # 16 x 32 full, 16 x 16 last
    add("first_16_64_7x7_wreg0_ragged", "plain", 8 * 3 + 1, 16, 64, 7, 7, 3, WREG0, "p3")       # 32 x 32 full, 16 x 32 last
    add("first_32_16_5x5_wreg0_ragged", "ctx", 8 * 2 + 1, 32, 16, 5, 5, 3, WREG0, "c1")         # 32 x 32 full, 16 x 16 last
    add("first_16_16_7x7_clipped", "plain", 3, 16, 16, 7, 7, 3, WREG0, "p0")                     # S clipped to B
    # gated mode: C = 6, 16, 20, 32 (padded and full tile pairs), both gated patch shapes
    for i, (C, cin, H, W, ks, B) in enumerate([(6, 6, 6, 6, 3, 17), (16, 16, 7, 7, 3, 41), (20, 20, 7, 7, 3, 9), (32, 32, 8, 8, 3, 2 * 256 * 4 + 6),
                                               (16, 16, 2, 2, 3, 3), (32, 32, 7, 7, 1, 12), (6, 6, 3, 3, 3, 8 * 256 + 1)]):
        add(f"gated_C{C}_{H}x{W}_k{ks}_B{B}", "gated", B, cin, C, H, W, ks, "", f"m{i % 2}")
    return rows


# ---- data --------------------------------------------------------------------------------------------------------------------
def _rng(c, what):
    key = f"{what}|{c.entry}|{c.cin}|{c.cout}|{c.H}|{c.W}|{c.ks}|{c.preset}"
    return np.random.default_rng(int.from_bytes(key.encode(), "little") % (1 << 63))


def _rows(c, what, shape, zeros=0.1):
    """[B, *shape] fp32, sample-sequential (the first n samples do not depend on B); a share of exact zeros, negatives"""
    r = _rng(c, what)
    v = r.standard_normal((c.B, *shape), dtype=np.float32)
    if zeros:
        v[r.random((c.B, *shape), dtype=np.float32) < zeros] = 0.0
    return torch.from_numpy(v)


def data(c):
    """every operand of the launch as CPU fp32 tensors (None where the form has none)"""
    HW = c.H * c.W
    r = _rng(c, "w")
    d = Case()
    d.w = torch.from_numpy(r.standard_normal((c.rows, c.cin, c.ks, c.ks), dtype=np.float32) / np.float32(np.sqrt(c.cin * c.ks * c.ks)))
    d.bias = torch.from_numpy(r.standard_normal(c.rows, dtype=np.float32)) if c.get("bias") else None
    if c.cout >= 48 and d.bias is not None:
        d.bias[48:] += 3.0                                           # (a bias missing there cannot hide)
    d.x = _rows(c, "x", (c.cin, c.H, c.W))
    d.in_mul = None
    if c.get("in_mul") == "rand":
        d.in_mul = torch.from_numpy((r.random((c.cin, c.H, c.W)) < 0.5).astype(np.float32))
    elif c.get("in_mul") == "chan":
        m = (r.random((c.cin, c.H, c.W)) < 0.5).astype(np.float32)
        m[::3] = 0.0                                                 # whole channels masked
        if c.cin > 1:
            m[1] = 1.0
        d.in_mul = torch.from_numpy(m)
    d.ctx = d.w_ctx = d.res_x = d.res_mul = d.gate_h = d.gate_mul = d.gate_add = d.gate_x = None
    if c.entry == "ctx":
        d.ctx = _rows(c, "ctx", (), zeros=0)
        d.w_ctx = torch.from_numpy(r.standard_normal((c.cout, c.ks * c.ks), dtype=np.float32) / 3)
    if c.entry == "res":
        d.res_x = _rows(c, "res_x", (c.cout, c.H, c.W))
        d.res_mul = torch.from_numpy((r.random((c.cout, c.H, c.W)) < 0.5).astype(np.float32))
    if c.entry in ("gate_mul", "gate_add"):
        d.gate_h = _rows(c, "gate_h", (c.cout, c.H, c.W))            # exact zeros included: the gate is > 0 ? 1 : slope
        if c.entry == "gate_add":
            d.gate_add = _rows(c, "gate_add", (c.cout, c.H, c.W))
        elif c.gate_mul:
            d.gate_mul = torch.from_numpy((r.random((c.cout, c.H, c.W)) < 0.6).astype(np.float32))
    if c.entry == "gated":
        d.gate_x = _rows(c, "gate_x", (c.C, c.H, c.W))
    assert HW == d.x.shape[2] * d.x.shape[3]
    return d


# ---- the weight planes, from the header's layout text -----------------------------------------------------------------------
def split3(w):
    """three bf16 planes with p0 + p1 + p2 == w up to the third residual (round-to-nearest residual split)"""
    h = w.to(torch.bfloat16)
    r = w - h.float()
    m = r.to(torch.bfloat16)
    lo = (r - m.float()).to(torch.bfloat16)
    return torch.stack([h, m, lo])


def gated_row_order(C):
    """packed row 32 t + r: value channel 16 t + r for r < 16, gate channel 16 t + r - 16 (original row C + ...) for r >= 16; -1: a zero row"""
    order = []
    for t in range((C + 15) // 16):
        for r in range(32):
            ch = 16 * t + (r % 16)
            order.append(-1 if ch >= C else (ch if r < 16 else C + ch))
    return order


def planes(c, w, bias):
    """(planes [3, coutp, kp] bf16, bias as the launch wants it): element [co][tap * cp + ci] = W[co, ci, tap / ks, tap % ks], channels
    padded to cp = ceil8(cin), K to kp = ceil32(ks ks cp), rows to coutp = ceil16(cout), zeros in all padding; gated mode packs the
    2 C rows (and the bias) interleaved in tiles of 16"""
    if c.entry == "gated":
        order = gated_row_order(c.C)
        wp = torch.zeros(len(order), *w.shape[1:])
        bp = torch.zeros(len(order)) if bias is not None else None
        for i, o in enumerate(order):
            if o >= 0:
                wp[i] = w[o]
                if bp is not None:
                    bp[i] = bias[o]
        w, bias = wp, bp
    rows, cin, ks = w.shape[0], w.shape[1], w.shape[2]
    cp, coutp = (cin + 7) // 8 * 8, (rows + 15) // 16 * 16
    kp = (ks * ks * cp + 31) // 32 * 32
    flat = torch.zeros(coutp, kp)
    tmp = torch.zeros(rows, ks * ks, cp)
    tmp[:, :, :cin] = w.reshape(rows, cin, ks * ks).permute(0, 2, 1)
    flat[:rows, :ks * ks * cp] = tmp.reshape(rows, -1)
    return split3(flat).contiguous(), bias


# ---- the statements -----------------------------------------------------------------------------------------------------------
def conv_same(a, w):
    """stride-1 zero-padded "same" convolution, one GEMM per tap added in tap order, in the operands' dtype"""
    B, cin, H, W = a.shape
    cout, ks = w.shape[0], w.shape[2]
    p = ks // 2
    ap = F.pad(a, (p, p, p, p)).permute(1, 0, 2, 3)
    acc = None
    for dy in range(ks):
        for dx in range(ks):
            t = w[:, :, dy, dx] @ ap[:, :, dy:dy + H, dx:dx + W].reshape(cin, -1)
            acc = t if acc is None else acc + t
    return acc.view(cout, B, H, W).permute(1, 0, 2, 3).contiguous()


def _leaky(v, act, slope):
    return torch.where(v > 0, v, v * slope) if act == LEAKY else v


def forward(c, d, dtype, defect=None):
    """(y, A) in `dtype` on d's device: the entry point's formula and the same formula with every term replaced by its magnitude"""
    t = lambda v: None if v is None else v.to(dtype)
    x, w, bias = t(d.x), t(d.w), t(d.bias)
    a = _leaky(x, c.get("in_act", NONE), c.get("in_slope", 0.0))
    if d.in_mul is not None:
        m = t(d.in_mul)
        a = a * (m.roll(1, 0) if defect == "in_mul_neighbour" else m)
    y = conv_same(a, w)
    A = conv_same(a.abs(), w.abs())
    if defect == "tap_dropped":                                      # the tap that reads pixel (0, 0) for output pixel (0, 1), first row, one channel
        y[0, 0, 0, 1] -= (w[0, :, 1, 0] * a[0, :, 0, 0]).sum()
    if bias is not None:
        b = bias.clone()
        if defect == "bias_missing_48":
            b[48:] = 0
        y = y + b.view(1, -1, 1, 1)
        A = A + bias.abs().view(1, -1, 1, 1)
    if c.entry == "ctx":
        ones = torch.ones(1, 1, c.H, c.W, dtype=dtype, device=x.device)
        wc = t(d.w_ctx).view(c.cout, 1, c.ks, c.ks)
        cx = t(d.ctx if c.ctx_stride else d.ctx[:1].expand(c.B)).view(-1, 1, 1, 1)
        y = y + cx * conv_same(ones, wc)
        A = A + cx.abs() * conv_same(ones, wc.abs())
    if c.entry in ("plain", "ctx"):
        return _leaky(y, c.out_act, c.out_slope), A                   # (|act(v) - act(v')| <= |v - v'| for slopes <= 1)
    if c.entry == "res":
        sign = -c.res_sign if defect == "res_sign" else c.res_sign
        return t(d.res_x) + sign * (t(d.res_mul) * y), t(d.res_x).abs() + t(d.res_mul).abs() * A
    if c.entry in ("gate_mul", "gate_add"):
        h = t(d.gate_h)
        g = torch.where((h >= 0) if defect == "gate_ge" else (h > 0), y, y * c.gate_slope)
        if c.entry == "gate_add":
            return t(d.gate_add) + g, t(d.gate_add).abs() + A
        return (g * t(d.gate_mul), A * t(d.gate_mul).abs()) if d.gate_mul is not None else (g, A)
    # gated mode: rows [0, C) values, [C, 2 C) gates; the error of val * sigmoid(gate) is at most dval + |val| / 4 * dgate, and the
    # evaluation of the sigmoid itself adds a few U * |val| * sigmoid
    val, gate = y[:, :c.C], y[:, c.C:]
    return t(d.gate_x) + val * torch.sigmoid(gate), t(d.gate_x).abs() + A[:, :c.C] + val.abs() * (1 + 0.25 * A[:, c.C:])


def reference(c, d):
    """(ref64, A64)"""
    return forward(c, d, torch.float64)


# ---- the checker -----------------------------------------------------------------------------------------------------------------
def guarded(c, device="cpu"):
    """the allocation y lies in: GUARD sentinels | B * cout * H * W | GUARD sentinels (+ 1 float when y starts off a 16-byte boundary)"""
    n = c.B * c.cout * c.H * c.W
    return torch.full((GUARD + n + GUARD,), sentinel(), dtype=torch.float32, device=device), n


def bits(t):
    return t.contiguous().view(torch.int32)


def measure(c, y, ref64, A64):
    """worst |y - ref64| / (U * A) over every element (0 / 0 counts as 0, x / 0 as inf)"""
    err = (y.double() - ref64).abs()
    ratio = torch.where(err == 0, torch.zeros_like(err), err / (U * A64))
    return ratio.max().item()


def check(c, buf, ref64, A64, bound=MARGIN * K32):
    """every finding of a launch's result buffer (see ``guarded``) against the fp64 statement; [] = the launch passes"""
    n = c.B * c.cout * c.H * c.W
    out = []
    s = torch.tensor([SENTINEL_BITS], dtype=torch.int32, device=buf.device)
    if not bool((bits(buf[:GUARD]) == s).all()):
        out.append("written in front of y")
    if not bool((bits(buf[GUARD + n:]) == s).all()):
        out.append("written behind y")
    y = buf[GUARD:GUARD + n].view(c.B, c.cout, c.H, c.W)
    left = bits(y) == s
    if bool(left.any()):
        b = int(left.view(c.B, -1).any(1).nonzero()[0])
        out.append(f"{int(left.sum())} elements of y left unwritten (first in sample {b})")
    if not bool(torch.isfinite(y).all()):
        out.append("non-finite values in y")
        return out
    err = (y.double() - ref64).abs()
    over = err > bound * U * A64
    if bool(over.any()):
        i = int(torch.where(over, err / (U * A64).clamp_min(1e-300), torch.zeros_like(err)).argmax())
        idx = np.unravel_index(i, tuple(y.shape))
        out.append(f"{int(over.sum())} elements over {bound} U A; worst at {idx}: got {y.flatten()[i].item()!r}, fp64 {ref64.flatten()[i].item()!r}, "
                   f"A {A64.flatten()[i].item()!r} ({(err.flatten()[i] / (U * A64.flatten()[i])).item():.2f} U A)")
    if err.max().item() > 3e-6 * max(1.0, ref64.abs().max().item()):
        out.append(f"max-norm bound: {err.max().item():.3e} > 3e-6 * max(1, {ref64.abs().max().item():.3e})")
    return out
