"""The gradient kernels of image training (usflows_amd/csrc/usf_image_grad.hip), launch by launch: the case tables, an fp64 and
two fp32 statements of every operation and a checker.  Importable without a GPU and without the library;
tests/test_image_grad_kernels_cpu.py proves the tables' coverage from the probes' answers (usf_conv_wgrad_variant,
usf_layernorm_channels_bwd_variant), tests/test_image_grad_kernels_gpu.py launches every row.

Weight-gradient rows (WG_ROWS): (name, B, cin, cout, H, W, ks, form, knobs, fault, rc, expect)
  form    FORMS: plain / mask_relu (0 / 1 in_mul, slope 0) / presub_leaky (pre_sub, slope 0.1) / nobias (db == NULL)
  knobs   tuning knobs in force ("conv_wgrad_blocks=2": the grid is capped at two blocks, "conv_wgrad_rsplit=0")
  fault   "" or what is wrong with the call: "xoff" (x one float off a 16-byte boundary), "short_ws" (workspace one float short)
  rc      the return code: 0 done, 1 not served, -2 refused; whenever rc != 0 nothing may be written
  expect  (kernel, CIT, COT, T, rsplit, blocks, rounds, rows_used, per, max_samples_per_wave) at 256 compute units and
          BLOCKS_PER_CU resident blocks per compute unit; kernel 1 = conv_wgrad_kernel, 2 = conv_wgrad_k1_kernel, 0 = not served.
          No row's grid reaches the occupancy cap (256 blocks at the least), so no expectation depends on the device's answer.
Rows named *_a / *_b are the two batch regimes: (a) default knobs, every wave takes at most one sample; (b) conv_wgrad_blocks=2
and the smallest B at which the waves take three and two samples and the last round is ragged (B = 2 nsw + 1, nsw = 8 / rsplit
samples in flight).
LayerNorm rows (LN_ROWS): (name, B, C, P, act, slope, rc, expect), expect = (kernel, width, blocks, rounds).
Gated-residual rows (GR_ROWS): (name, B, CP).  Context rows (CTX_ROWS): (name, B, cout, H, W, ks, ctx_stride).
"""
import numpy as np
import torch
import torch.nn.functional as F

from conv_kernel_cases import GUARD, MARGIN, SENTINEL_BITS, U, Case, bits, knobs, sentinel  # noqa: F401  (MARGIN = 4: the same margin)

CUS, BLOCKS_PER_CU = 256, 1
LEAKY, NONE = 1, 0

# max over the tables of |fp32 statement - fp64 statement| / (U * A), measured on a CPU (tests/test_image_grad_kernels_cpu.py
# asserts that the fp32 statements stay inside), rounded up in the second digit; the row that set each.  For the sums over
# the batch the larger of two fp32 statements: torch's einsum / sum, and a strictly sequential accumulation over the samples.
K = {
    "wg_dW": 4.3,        # 4.276  t1_2x3_nobias_b (einsum)
    "wg_db": 1.4,        # 1.397  t1_3x4_presub_leaky_b (sum)
    "ln_dx": 4.0,        # 3.980  ln_cap_k1_C3
    "ln_dgamma": 1.2,    # 1.170  ln_C47_B3_P7 (sum)
    "ln_dbeta": 1.3,     # 1.249  ln_C49_B3_P7 (sum)
    "gr_dvg": 3.9,       # 3.898  gr_cap
    "ctx_dw": 2.4,       # 2.371  ctx_7x7_k3_B1_c5 (einsum)
}
MAXNORM = {"wg_dW": 2e-6, "wg_db": 2e-6, "ln_dx": 1e-5, "ln_dgamma": 1e-5, "ln_dbeta": 1e-5, "gr_dvg": 1e-6, "ctx_dw": 1e-5}

FORMS = {
    "plain": dict(mask=False, pre_sub=False, act=NONE, slope=0.0, bias=True),
    "mask_relu": dict(mask=True, pre_sub=False, act=LEAKY, slope=0.0, bias=True),
    "presub_leaky": dict(mask=False, pre_sub=True, act=LEAKY, slope=0.1, bias=True),
    "nobias": dict(mask=False, pre_sub=False, act=NONE, slope=0.0, bias=False),
}
T9_TILES = [(1, 1), (1, 2), (2, 1), (2, 2), (3, 2), (2, 3), (1, 3), (3, 1)]                 # USF_WG_INSTANCES, T = 9
T1_TILES = [(i, j) for i in range(1, 5) for j in range(1, 5)]                            # ... T = 1 and USF_WG_K1_INSTANCES
PICTURES = [(7, 7), (8, 8), (1, 2), (2, 2), (3, 5), (32, 2), (2, 32), (1, 64), (21, 3), (9, 7), (4, 16)]
NCH_PICTURES = {3: (2, 5), 4: (3, 4), 7: (4, 6), 8: (4, 7)}                                # kernel 3: nch through the picture


def direct_pictures():
    """for every H W in 49..64: (the most square factorisation with W >= 2, the single row 1 x HW)"""
    out = []
    for hw in range(49, 65):
        h = max(h for h in range(1, 9) if hw % h == 0 and hw // h >= 2)
        out.append(((h, hw // h), (1, hw)))
    return out


# ---- the tables (generated: generate_rows below with the probes' answers; the CPU file asserts they are exactly that) ---------
# TABLES-BEGIN
WG_ROWS = [
    ('t9_1x1_plain_a', 9, 16, 16, 7, 7, 3, 'plain', '', '', 0, (1, 1, 1, 9, 4, 9, 1, 1, 36, 1)),
    ('t9_1x1_mask_relu_b', 5, 16, 16, 8, 8, 3, 'mask_relu', 'conv_wgrad_blocks=2', '', 0, (1, 1, 1, 9, 4, 2, 1, 1, 8, 3)),
    ('t9_1x1_presub_leaky_a', 9, 16, 16, 3, 5, 3, 'presub_leaky', '', '', 0, (1, 1, 1, 9, 2, 5, 1, 1, 20, 1)),
    ('t9_1x1_nobias_b', 5, 16, 16, 6, 8, 3, 'nobias', 'conv_wgrad_blocks=2', '', 0, (1, 1, 1, 9, 4, 2, 1, 1, 8, 3)),
    ('t9_1x2_plain_b', 5, 16, 32, 9, 7, 3, 'plain', 'conv_wgrad_blocks=2', '', 0, (1, 1, 2, 9, 4, 2, 1, 1, 8, 3)),
    ('t9_1x2_mask_relu_a', 9, 16, 32, 2, 2, 3, 'mask_relu', '', '', 0, (1, 1, 2, 9, 1, 3, 1, 1, 12, 1)),
    ('t9_1x2_presub_leaky_b', 5, 16, 32, 4, 16, 3, 'presub_leaky', 'conv_wgrad_blocks=2', '', 0, (1, 1, 2, 9, 4, 2, 1, 1, 8, 3)),
    ('t9_1x2_nobias_a', 9, 16, 32, 7, 7, 3, 'nobias', '', '', 0, (1, 1, 2, 9, 4, 9, 1, 1, 36, 1)),
    ('t9_2x1_plain_a', 9, 32, 16, 8, 8, 3, 'plain', '', '', 0, (1, 2, 1, 9, 4, 9, 1, 1, 36, 1)),
    ('t9_2x1_mask_relu_b', 9, 32, 16, 3, 5, 3, 'mask_relu', 'conv_wgrad_blocks=2', '', 0, (1, 2, 1, 9, 2, 2, 1, 1, 8, 3)),
    ('t9_2x1_presub_leaky_a', 9, 32, 16, 6, 8, 3, 'presub_leaky', '', '', 0, (1, 2, 1, 9, 4, 9, 1, 1, 36, 1)),
    ('t9_2x1_nobias_b', 5, 32, 16, 9, 7, 3, 'nobias', 'conv_wgrad_blocks=2', '', 0, (1, 2, 1, 9, 4, 2, 1, 1, 8, 3)),
    ('t9_2x2_plain_b', 17, 32, 32, 2, 2, 3, 'plain', 'conv_wgrad_blocks=2', '', 0, (1, 2, 2, 9, 1, 2, 1, 1, 8, 3)),
    ('t9_2x2_mask_relu_a', 9, 32, 32, 4, 16, 3, 'mask_relu', '', '', 0, (1, 2, 2, 9, 4, 9, 1, 1, 36, 1)),
    ('t9_2x2_presub_leaky_b', 5, 32, 32, 7, 7, 3, 'presub_leaky', 'conv_wgrad_blocks=2', '', 0, (1, 2, 2, 9, 4, 2, 1, 1, 8, 3)),
    ('t9_2x2_nobias_a', 9, 32, 32, 8, 8, 3, 'nobias', '', '', 0, (1, 2, 2, 9, 4, 9, 1, 1, 36, 1)),
    ('t9_3x2_plain_a', 9, 48, 32, 3, 5, 3, 'plain', '', '', 0, (1, 3, 2, 9, 2, 5, 1, 1, 20, 1)),
    ('t9_3x2_mask_relu_b', 5, 48, 32, 6, 8, 3, 'mask_relu', 'conv_wgrad_blocks=2', '', 0, (1, 3, 2, 9, 4, 2, 1, 1, 8, 3)),
    ('t9_3x2_presub_leaky_a', 9, 48, 32, 9, 7, 3, 'presub_leaky', '', '', 0, (1, 3, 2, 9, 4, 9, 1, 1, 36, 1)),
    ('t9_3x2_nobias_b', 17, 48, 32, 2, 2, 3, 'nobias', 'conv_wgrad_blocks=2', '', 0, (1, 3, 2, 9, 1, 2, 1, 1, 8, 3)),
    ('t9_2x3_plain_b', 5, 32, 48, 4, 16, 3, 'plain', 'conv_wgrad_blocks=2', '', 0, (1, 2, 3, 9, 4, 2, 1, 1, 8, 3)),
    ('t9_2x3_mask_relu_a', 9, 32, 48, 7, 7, 3, 'mask_relu', '', '', 0, (1, 2, 3, 9, 4, 9, 1, 1, 36, 1)),
    ('t9_2x3_presub_leaky_b', 5, 32, 48, 8, 8, 3, 'presub_leaky', 'conv_wgrad_blocks=2', '', 0, (1, 2, 3, 9, 4, 2, 1, 1, 8, 3)),
    ('t9_2x3_nobias_a', 9, 32, 48, 3, 5, 3, 'nobias', '', '', 0, (1, 2, 3, 9, 2, 5, 1, 1, 20, 1)),
    ('t9_1x3_plain_a', 9, 16, 48, 6, 8, 3, 'plain', '', '', 0, (1, 1, 3, 9, 4, 9, 1, 1, 36, 1)),
    ('t9_1x3_mask_relu_b', 5, 16, 48, 9, 7, 3, 'mask_relu', 'conv_wgrad_blocks=2', '', 0, (1, 1, 3, 9, 4, 2, 1, 1, 8, 3)),
    ('t9_1x3_presub_leaky_a', 9, 16, 48, 2, 2, 3, 'presub_leaky', '', '', 0, (1, 1, 3, 9, 1, 3, 1, 1, 12, 1)),
    ('t9_1x3_nobias_b', 5, 16, 48, 4, 16, 3, 'nobias', 'conv_wgrad_blocks=2', '', 0, (1, 1, 3, 9, 4, 2, 1, 1, 8, 3)),
    ('t9_3x1_plain_b', 5, 48, 16, 7, 7, 3, 'plain', 'conv_wgrad_blocks=2', '', 0, (1, 3, 1, 9, 4, 2, 1, 1, 8, 3)),
    ('t9_3x1_mask_relu_a', 9, 48, 16, 8, 8, 3, 'mask_relu', '', '', 0, (1, 3, 1, 9, 4, 9, 1, 1, 36, 1)),
    ('t9_3x1_presub_leaky_b', 9, 48, 16, 3, 5, 3, 'presub_leaky', 'conv_wgrad_blocks=2', '', 0, (1, 3, 1, 9, 2, 2, 1, 1, 8, 3)),
    ('t9_3x1_nobias_a', 9, 48, 16, 6, 8, 3, 'nobias', '', '', 0, (1, 3, 1, 9, 4, 9, 1, 1, 36, 1)),
    ('t1_1x1_plain_a', 9, 16, 16, 6, 8, 1, 'plain', '', '', 0, (1, 1, 1, 1, 1, 3, 1, 1, 12, 1)),
    ('t1_1x1_mask_relu_b', 17, 16, 16, 3, 5, 1, 'mask_relu', 'conv_wgrad_blocks=2', '', 0, (1, 1, 1, 1, 1, 2, 1, 1, 8, 3)),
    ('t1_1x1_presub_leaky_a', 9, 16, 16, 4, 12, 1, 'presub_leaky', '', '', 0, (1, 1, 1, 1, 1, 3, 1, 1, 12, 1)),
    ('t1_1x1_nobias_b', 17, 16, 16, 2, 2, 1, 'nobias', 'conv_wgrad_blocks=2', '', 0, (1, 1, 1, 1, 1, 2, 1, 1, 8, 3)),
    ('t1_1x2_plain_b', 17, 16, 32, 1, 2, 1, 'plain', 'conv_wgrad_blocks=2', '', 0, (1, 1, 2, 1, 1, 2, 1, 1, 8, 3)),
    ('t1_1x2_mask_relu_a', 9, 16, 32, 5, 9, 1, 'mask_relu', '', '', 0, (1, 1, 2, 1, 1, 3, 1, 1, 12, 1)),
    ('t1_1x2_presub_leaky_b', 17, 16, 32, 6, 8, 1, 'presub_leaky', 'conv_wgrad_blocks=2', '', 0, (1, 1, 2, 1, 1, 2, 1, 1, 8, 3)),
    ('t1_1x2_nobias_a', 9, 16, 32, 3, 5, 1, 'nobias', '', '', 0, (1, 1, 2, 1, 1, 3, 1, 1, 12, 1)),
    ('t1_1x3_plain_a', 9, 16, 48, 4, 12, 1, 'plain', '', '', 0, (1, 1, 3, 1, 1, 3, 1, 1, 12, 1)),
    ('t1_1x3_mask_relu_b', 17, 16, 48, 2, 2, 1, 'mask_relu', 'conv_wgrad_blocks=2', '', 0, (1, 1, 3, 1, 1, 2, 1, 1, 8, 3)),
    ('t1_1x3_presub_leaky_a', 9, 16, 48, 1, 2, 1, 'presub_leaky', '', '', 0, (1, 1, 3, 1, 1, 3, 1, 1, 12, 1)),
    ('t1_1x3_nobias_b', 17, 16, 48, 5, 9, 1, 'nobias', 'conv_wgrad_blocks=2', '', 0, (1, 1, 3, 1, 1, 2, 1, 1, 8, 3)),
    ('t1_1x4_plain_b', 17, 16, 64, 6, 8, 1, 'plain', 'conv_wgrad_blocks=2', '', 0, (1, 1, 4, 1, 1, 2, 1, 1, 8, 3)),
    ('t1_1x4_mask_relu_a', 9, 16, 64, 3, 5, 1, 'mask_relu', '', '', 0, (1, 1, 4, 1, 1, 3, 1, 1, 12, 1)),
    ('t1_1x4_presub_leaky_b', 17, 16, 64, 4, 12, 1, 'presub_leaky', 'conv_wgrad_blocks=2', '', 0, (1, 1, 4, 1, 1, 2, 1, 1, 8, 3)),
    ('t1_1x4_nobias_a', 9, 16, 64, 2, 2, 1, 'nobias', '', '', 0, (1, 1, 4, 1, 1, 3, 1, 1, 12, 1)),
    ('t1_2x1_plain_a', 9, 32, 16, 1, 2, 1, 'plain', '', '', 0, (1, 2, 1, 1, 1, 3, 1, 1, 12, 1)),
    ('t1_2x1_mask_relu_b', 17, 32, 16, 5, 9, 1, 'mask_relu', 'conv_wgrad_blocks=2', '', 0, (1, 2, 1, 1, 1, 2, 1, 1, 8, 3)),
    ('t1_2x1_presub_leaky_a', 9, 32, 16, 6, 8, 1, 'presub_leaky', '', '', 0, (1, 2, 1, 1, 1, 3, 1, 1, 12, 1)),
    ('t1_2x1_nobias_b', 17, 32, 16, 3, 5, 1, 'nobias', 'conv_wgrad_blocks=2', '', 0, (1, 2, 1, 1, 1, 2, 1, 1, 8, 3)),
    ('t1_2x2_plain_b', 17, 32, 32, 4, 12, 1, 'plain', 'conv_wgrad_blocks=2', '', 0, (1, 2, 2, 1, 1, 2, 1, 1, 8, 3)),
    ('t1_2x2_mask_relu_a', 9, 32, 32, 2, 2, 1, 'mask_relu', '', '', 0, (1, 2, 2, 1, 1, 3, 1, 1, 12, 1)),
    ('t1_2x2_presub_leaky_b', 17, 32, 32, 1, 2, 1, 'presub_leaky', 'conv_wgrad_blocks=2', '', 0, (1, 2, 2, 1, 1, 2, 1, 1, 8, 3)),
    ('t1_2x2_nobias_a', 9, 32, 32, 5, 9, 1, 'nobias', '', '', 0, (1, 2, 2, 1, 1, 3, 1, 1, 12, 1)),
    ('t1_2x3_plain_a', 9, 32, 48, 6, 8, 1, 'plain', '', '', 0, (1, 2, 3, 1, 1, 3, 1, 1, 12, 1)),
    ('t1_2x3_mask_relu_b', 17, 32, 48, 3, 5, 1, 'mask_relu', 'conv_wgrad_blocks=2', '', 0, (1, 2, 3, 1, 1, 2, 1, 1, 8, 3)),
    ('t1_2x3_presub_leaky_a', 9, 32, 48, 4, 12, 1, 'presub_leaky', '', '', 0, (1, 2, 3, 1, 1, 3, 1, 1, 12, 1)),
    ('t1_2x3_nobias_b', 17, 32, 48, 2, 2, 1, 'nobias', 'conv_wgrad_blocks=2', '', 0, (1, 2, 3, 1, 1, 2, 1, 1, 8, 3)),
    ('t1_2x4_plain_b', 17, 32, 64, 1, 2, 1, 'plain', 'conv_wgrad_blocks=2', '', 0, (1, 2, 4, 1, 1, 2, 1, 1, 8, 3)),
    ('t1_2x4_mask_relu_a', 9, 32, 64, 5, 9, 1, 'mask_relu', '', '', 0, (1, 2, 4, 1, 1, 3, 1, 1, 12, 1)),
    ('t1_2x4_presub_leaky_b', 17, 32, 64, 6, 8, 1, 'presub_leaky', 'conv_wgrad_blocks=2', '', 0, (1, 2, 4, 1, 1, 2, 1, 1, 8, 3)),
    ('t1_2x4_nobias_a', 9, 32, 64, 3, 5, 1, 'nobias', '', '', 0, (1, 2, 4, 1, 1, 3, 1, 1, 12, 1)),
    ('t1_3x1_plain_a', 9, 48, 16, 4, 12, 1, 'plain', '', '', 0, (1, 3, 1, 1, 1, 3, 1, 1, 12, 1)),
    ('t1_3x1_mask_relu_b', 17, 48, 16, 2, 2, 1, 'mask_relu', 'conv_wgrad_blocks=2', '', 0, (1, 3, 1, 1, 1, 2, 1, 1, 8, 3)),
    ('t1_3x1_presub_leaky_a', 9, 48, 16, 1, 2, 1, 'presub_leaky', '', '', 0, (1, 3, 1, 1, 1, 3, 1, 1, 12, 1)),
    ('t1_3x1_nobias_b', 17, 48, 16, 5, 9, 1, 'nobias', 'conv_wgrad_blocks=2', '', 0, (1, 3, 1, 1, 1, 2, 1, 1, 8, 3)),
    ('t1_3x2_plain_b', 17, 48, 32, 6, 8, 1, 'plain', 'conv_wgrad_blocks=2', '', 0, (1, 3, 2, 1, 1, 2, 1, 1, 8, 3)),
    ('t1_3x2_mask_relu_a', 9, 48, 32, 3, 5, 1, 'mask_relu', '', '', 0, (1, 3, 2, 1, 1, 3, 1, 1, 12, 1)),
    ('t1_3x2_presub_leaky_b', 17, 48, 32, 4, 12, 1, 'presub_leaky', 'conv_wgrad_blocks=2', '', 0, (1, 3, 2, 1, 1, 2, 1, 1, 8, 3)),
    ('t1_3x2_nobias_a', 9, 48, 32, 2, 2, 1, 'nobias', '', '', 0, (1, 3, 2, 1, 1, 3, 1, 1, 12, 1)),
    ('t1_3x3_plain_a', 9, 48, 48, 1, 2, 1, 'plain', '', '', 0, (1, 3, 3, 1, 1, 3, 1, 1, 12, 1)),
    ('t1_3x3_mask_relu_b', 17, 48, 48, 5, 9, 1, 'mask_relu', 'conv_wgrad_blocks=2', '', 0, (1, 3, 3, 1, 1, 2, 1, 1, 8, 3)),
    ('t1_3x3_presub_leaky_a', 9, 48, 48, 6, 8, 1, 'presub_leaky', '', '', 0, (1, 3, 3, 1, 1, 3, 1, 1, 12, 1)),
    ('t1_3x3_nobias_b', 17, 48, 48, 3, 5, 1, 'nobias', 'conv_wgrad_blocks=2', '', 0, (1, 3, 3, 1, 1, 2, 1, 1, 8, 3)),
    ('t1_3x4_plain_b', 17, 48, 64, 4, 12, 1, 'plain', 'conv_wgrad_blocks=2', '', 0, (1, 3, 4, 1, 1, 2, 1, 1, 8, 3)),
    ('t1_3x4_mask_relu_a', 9, 48, 64, 2, 2, 1, 'mask_relu', '', '', 0, (1, 3, 4, 1, 1, 3, 1, 1, 12, 1)),
    ('t1_3x4_presub_leaky_b', 17, 48, 64, 1, 2, 1, 'presub_leaky', 'conv_wgrad_blocks=2', '', 0, (1, 3, 4, 1, 1, 2, 1, 1, 8, 3)),
    ('t1_3x4_nobias_a', 9, 48, 64, 5, 9, 1, 'nobias', '', '', 0, (1, 3, 4, 1, 1, 3, 1, 1, 12, 1)),
    ('t1_4x1_plain_a', 9, 64, 16, 6, 8, 1, 'plain', '', '', 0, (1, 4, 1, 1, 1, 3, 1, 1, 12, 1)),
    ('t1_4x1_mask_relu_b', 17, 64, 16, 3, 5, 1, 'mask_relu', 'conv_wgrad_blocks=2', '', 0, (1, 4, 1, 1, 1, 2, 1, 1, 8, 3)),
    ('t1_4x1_presub_leaky_a', 9, 64, 16, 4, 12, 1, 'presub_leaky', '', '', 0, (1, 4, 1, 1, 1, 3, 1, 1, 12, 1)),
    ('t1_4x1_nobias_b', 17, 64, 16, 2, 2, 1, 'nobias', 'conv_wgrad_blocks=2', '', 0, (1, 4, 1, 1, 1, 2, 1, 1, 8, 3)),
    ('t1_4x2_plain_b', 17, 64, 32, 1, 2, 1, 'plain', 'conv_wgrad_blocks=2', '', 0, (1, 4, 2, 1, 1, 2, 1, 1, 8, 3)),
    ('t1_4x2_mask_relu_a', 9, 64, 32, 5, 9, 1, 'mask_relu', '', '', 0, (1, 4, 2, 1, 1, 3, 1, 1, 12, 1)),
    ('t1_4x2_presub_leaky_b', 17, 64, 32, 6, 8, 1, 'presub_leaky', 'conv_wgrad_blocks=2', '', 0, (1, 4, 2, 1, 1, 2, 1, 1, 8, 3)),
    ('t1_4x2_nobias_a', 9, 64, 32, 3, 5, 1, 'nobias', '', '', 0, (1, 4, 2, 1, 1, 3, 1, 1, 12, 1)),
    ('t1_4x3_plain_a', 9, 64, 48, 4, 12, 1, 'plain', '', '', 0, (1, 4, 3, 1, 1, 3, 1, 1, 12, 1)),
    ('t1_4x3_mask_relu_b', 17, 64, 48, 2, 2, 1, 'mask_relu', 'conv_wgrad_blocks=2', '', 0, (1, 4, 3, 1, 1, 2, 1, 1, 8, 3)),
    ('t1_4x3_presub_leaky_a', 9, 64, 48, 1, 2, 1, 'presub_leaky', '', '', 0, (1, 4, 3, 1, 1, 3, 1, 1, 12, 1)),
    ('t1_4x3_nobias_b', 17, 64, 48, 5, 9, 1, 'nobias', 'conv_wgrad_blocks=2', '', 0, (1, 4, 3, 1, 1, 2, 1, 1, 8, 3)),
    ('t1_4x4_plain_b', 17, 64, 64, 6, 8, 1, 'plain', 'conv_wgrad_blocks=2', '', 0, (1, 4, 4, 1, 1, 2, 1, 1, 8, 3)),
    ('t1_4x4_mask_relu_a', 9, 64, 64, 3, 5, 1, 'mask_relu', '', '', 0, (1, 4, 4, 1, 1, 3, 1, 1, 12, 1)),
    ('t1_4x4_presub_leaky_b', 17, 64, 64, 4, 12, 1, 'presub_leaky', 'conv_wgrad_blocks=2', '', 0, (1, 4, 4, 1, 1, 2, 1, 1, 8, 3)),
    ('t1_4x4_nobias_a', 9, 64, 64, 2, 2, 1, 'nobias', '', '', 0, (1, 4, 4, 1, 1, 3, 1, 1, 12, 1)),
    ('k1_1x1_plain_a', 9, 16, 16, 7, 7, 1, 'plain', '', '', 0, (2, 1, 1, 1, 1, 3, 1, 1, 12, 1)),
    ('k1_1x1_presub_leaky_b', 17, 16, 16, 5, 10, 1, 'presub_leaky', 'conv_wgrad_blocks=2', '', 0, (2, 1, 1, 1, 1, 2, 1, 1, 8, 3)),
    ('k1_1x2_plain_b', 17, 16, 32, 3, 17, 1, 'plain', 'conv_wgrad_blocks=2', '', 0, (2, 1, 2, 1, 1, 2, 1, 1, 8, 3)),
    ('k1_1x2_presub_leaky_a', 9, 16, 32, 4, 13, 1, 'presub_leaky', '', '', 0, (2, 1, 2, 1, 1, 3, 1, 1, 12, 1)),
    ('k1_1x3_plain_a', 9, 16, 48, 1, 53, 1, 'plain', '', '', 0, (2, 1, 3, 1, 1, 3, 1, 1, 12, 1)),
    ('k1_1x3_presub_leaky_b', 17, 16, 48, 6, 9, 1, 'presub_leaky', 'conv_wgrad_blocks=2', '', 0, (2, 1, 3, 1, 1, 2, 1, 1, 8, 3)),
    ('k1_1x4_plain_b', 17, 16, 64, 5, 11, 1, 'plain', 'conv_wgrad_blocks=2', '', 0, (2, 1, 4, 1, 1, 2, 1, 1, 8, 3)),
    ('k1_1x4_presub_leaky_a', 9, 16, 64, 8, 7, 1, 'presub_leaky', '', '', 0, (2, 1, 4, 1, 1, 3, 1, 1, 12, 1)),
    ('k1_2x1_plain_a', 9, 32, 16, 3, 19, 1, 'plain', '', '', 0, (2, 2, 1, 1, 1, 3, 1, 1, 12, 1)),
    ('k1_2x1_presub_leaky_b', 17, 32, 16, 2, 29, 1, 'presub_leaky', 'conv_wgrad_blocks=2', '', 0, (2, 2, 1, 1, 1, 2, 1, 1, 8, 3)),
    ('k1_2x2_plain_b', 17, 32, 32, 1, 59, 1, 'plain', 'conv_wgrad_blocks=2', '', 0, (2, 2, 2, 1, 1, 2, 1, 1, 8, 3)),
    ('k1_2x2_presub_leaky_a', 9, 32, 32, 6, 10, 1, 'presub_leaky', '', '', 0, (2, 2, 2, 1, 1, 3, 1, 1, 12, 1)),
    ('k1_2x3_plain_a', 9, 32, 48, 1, 61, 1, 'plain', '', '', 0, (2, 2, 3, 1, 1, 3, 1, 1, 12, 1)),
    ('k1_2x3_presub_leaky_b', 17, 32, 48, 2, 31, 1, 'presub_leaky', 'conv_wgrad_blocks=2', '', 0, (2, 2, 3, 1, 1, 2, 1, 1, 8, 3)),
    ('k1_2x4_plain_b', 17, 32, 64, 7, 9, 1, 'plain', 'conv_wgrad_blocks=2', '', 0, (2, 2, 4, 1, 1, 2, 1, 1, 8, 3)),
    ('k1_2x4_presub_leaky_a', 9, 32, 64, 8, 8, 1, 'presub_leaky', '', '', 0, (2, 2, 4, 1, 1, 3, 1, 1, 12, 1)),
    ('k1_3x1_plain_a', 9, 48, 16, 1, 49, 1, 'plain', '', '', 0, (2, 3, 1, 1, 1, 3, 1, 1, 12, 1)),
    ('k1_3x1_presub_leaky_b', 17, 48, 16, 1, 50, 1, 'presub_leaky', 'conv_wgrad_blocks=2', '', 0, (2, 3, 1, 1, 1, 2, 1, 1, 8, 3)),
    ('k1_3x2_plain_b', 17, 48, 32, 1, 51, 1, 'plain', 'conv_wgrad_blocks=2', '', 0, (2, 3, 2, 1, 1, 2, 1, 1, 8, 3)),
    ('k1_3x2_presub_leaky_a', 9, 48, 32, 1, 52, 1, 'presub_leaky', '', '', 0, (2, 3, 2, 1, 1, 3, 1, 1, 12, 1)),
    ('k1_3x3_plain_a', 9, 48, 48, 1, 53, 1, 'plain', '', '', 0, (2, 3, 3, 1, 1, 3, 1, 1, 12, 1)),
    ('k1_3x3_presub_leaky_b', 17, 48, 48, 1, 54, 1, 'presub_leaky', 'conv_wgrad_blocks=2', '', 0, (2, 3, 3, 1, 1, 2, 1, 1, 8, 3)),
    ('k1_3x4_plain_b', 17, 48, 64, 1, 55, 1, 'plain', 'conv_wgrad_blocks=2', '', 0, (2, 3, 4, 1, 1, 2, 1, 1, 8, 3)),
    ('k1_3x4_presub_leaky_a', 9, 48, 64, 1, 56, 1, 'presub_leaky', '', '', 0, (2, 3, 4, 1, 1, 3, 1, 1, 12, 1)),
    ('k1_4x1_plain_a', 9, 64, 16, 1, 57, 1, 'plain', '', '', 0, (2, 4, 1, 1, 1, 3, 1, 1, 12, 1)),
    ('k1_4x1_presub_leaky_b', 17, 64, 16, 1, 58, 1, 'presub_leaky', 'conv_wgrad_blocks=2', '', 0, (2, 4, 1, 1, 1, 2, 1, 1, 8, 3)),
    ('k1_4x2_plain_b', 17, 64, 32, 1, 59, 1, 'plain', 'conv_wgrad_blocks=2', '', 0, (2, 4, 2, 1, 1, 2, 1, 1, 8, 3)),
    ('k1_4x2_presub_leaky_a', 9, 64, 32, 1, 60, 1, 'presub_leaky', '', '', 0, (2, 4, 2, 1, 1, 3, 1, 1, 12, 1)),
    ('k1_4x3_plain_a', 9, 64, 48, 1, 61, 1, 'plain', '', '', 0, (2, 4, 3, 1, 1, 3, 1, 1, 12, 1)),
    ('k1_4x3_presub_leaky_b', 17, 64, 48, 1, 62, 1, 'presub_leaky', 'conv_wgrad_blocks=2', '', 0, (2, 4, 3, 1, 1, 2, 1, 1, 8, 3)),
    ('k1_4x4_plain_b', 17, 64, 64, 1, 63, 1, 'plain', 'conv_wgrad_blocks=2', '', 0, (2, 4, 4, 1, 1, 2, 1, 1, 8, 3)),
    ('k1_4x4_presub_leaky_a', 9, 64, 64, 1, 64, 1, 'presub_leaky', '', '', 0, (2, 4, 4, 1, 1, 3, 1, 1, 12, 1)),
    ('pic_7x7_k3', 9, 16, 16, 7, 7, 3, 'mask_relu', '', '', 0, (1, 1, 1, 9, 4, 9, 1, 1, 36, 1)),
    ('pic_7x7_k1', 9, 16, 16, 7, 7, 1, 'mask_relu', '', '', 0, (1, 1, 1, 1, 1, 3, 1, 1, 12, 1)),
    ('pic_8x8_k3', 9, 16, 16, 8, 8, 3, 'mask_relu', '', '', 0, (1, 1, 1, 9, 4, 9, 1, 1, 36, 1)),
    ('pic_8x8_k1', 9, 16, 16, 8, 8, 1, 'mask_relu', '', '', 0, (1, 1, 1, 1, 1, 3, 1, 1, 12, 1)),
    ('pic_1x2_k3', 9, 16, 16, 1, 2, 3, 'mask_relu', '', '', 0, (1, 1, 1, 9, 1, 3, 1, 1, 12, 1)),
    ('pic_1x2_k1', 9, 16, 16, 1, 2, 1, 'mask_relu', '', '', 0, (1, 1, 1, 1, 1, 3, 1, 1, 12, 1)),
    ('pic_2x2_k3', 9, 16, 16, 2, 2, 3, 'mask_relu', '', '', 0, (1, 1, 1, 9, 1, 3, 1, 1, 12, 1)),
    ('pic_2x2_k1', 9, 16, 16, 2, 2, 1, 'mask_relu', '', '', 0, (1, 1, 1, 1, 1, 3, 1, 1, 12, 1)),
    ('pic_3x5_k3', 9, 16, 16, 3, 5, 3, 'mask_relu', '', '', 0, (1, 1, 1, 9, 2, 5, 1, 1, 20, 1)),
    ('pic_3x5_k1', 9, 16, 16, 3, 5, 1, 'mask_relu', '', '', 0, (1, 1, 1, 1, 1, 3, 1, 1, 12, 1)),
    ('pic_32x2_k3', 9, 16, 16, 32, 2, 3, 'mask_relu', '', '', 0, (1, 1, 1, 9, 4, 9, 1, 1, 36, 1)),
    ('pic_32x2_k1', 9, 16, 16, 32, 2, 1, 'mask_relu', '', '', 0, (1, 1, 1, 1, 1, 3, 1, 1, 12, 1)),
    ('pic_2x32_k3', 9, 16, 16, 2, 32, 3, 'mask_relu', '', '', 0, (1, 1, 1, 9, 4, 9, 1, 1, 36, 1)),
    ('pic_2x32_k1', 9, 16, 16, 2, 32, 1, 'mask_relu', '', '', 0, (1, 1, 1, 1, 1, 3, 1, 1, 12, 1)),
    ('pic_1x64_k3', 9, 16, 16, 1, 64, 3, 'mask_relu', '', '', 0, (1, 1, 1, 9, 4, 9, 1, 1, 36, 1)),
    ('pic_1x64_k1', 9, 16, 16, 1, 64, 1, 'mask_relu', '', '', 0, (1, 1, 1, 1, 1, 3, 1, 1, 12, 1)),
    ('pic_21x3_k3', 9, 16, 16, 21, 3, 3, 'mask_relu', '', '', 0, (1, 1, 1, 9, 4, 9, 1, 1, 36, 1)),
    ('pic_21x3_k1', 9, 16, 16, 21, 3, 1, 'mask_relu', '', '', 0, (1, 1, 1, 1, 1, 3, 1, 1, 12, 1)),
    ('pic_9x7_k3', 9, 16, 16, 9, 7, 3, 'mask_relu', '', '', 0, (1, 1, 1, 9, 4, 9, 1, 1, 36, 1)),
    ('pic_9x7_k1', 9, 16, 16, 9, 7, 1, 'mask_relu', '', '', 0, (1, 1, 1, 1, 1, 3, 1, 1, 12, 1)),
    ('pic_4x16_k3', 9, 16, 16, 4, 16, 3, 'mask_relu', '', '', 0, (1, 1, 1, 9, 4, 9, 1, 1, 36, 1)),
    ('pic_4x16_k1', 9, 16, 16, 4, 16, 1, 'mask_relu', '', '', 0, (1, 1, 1, 1, 1, 3, 1, 1, 12, 1)),
    ('pic_6x8_k1_unmasked_48_pixels', 9, 32, 16, 6, 8, 1, 'presub_leaky', '', '', 0, (1, 2, 1, 1, 1, 3, 1, 1, 12, 1)),
    ('rs_B64', 64, 16, 16, 7, 7, 3, 'plain', '', '', 0, (1, 1, 1, 9, 4, 64, 2, 16, 16, 1)),
    ('rs_B65', 65, 16, 16, 7, 7, 3, 'plain', '', '', 0, (1, 1, 1, 9, 2, 33, 2, 9, 15, 1)),
    ('rs_B128', 128, 16, 16, 7, 7, 3, 'plain', '', '', 0, (1, 1, 1, 9, 2, 64, 2, 16, 16, 1)),
    ('rs_B129', 129, 16, 16, 7, 7, 3, 'plain', '', '', 0, (1, 1, 1, 9, 1, 33, 2, 9, 15, 1)),
    ('rs_nch3', 9, 16, 32, 2, 5, 3, 'presub_leaky', '', '', 0, (1, 1, 2, 9, 1, 3, 1, 1, 12, 1)),
    ('rs_nch4', 9, 16, 32, 3, 4, 3, 'presub_leaky', '', '', 0, (1, 1, 2, 9, 2, 5, 1, 1, 20, 1)),
    ('rs_nch7', 9, 16, 32, 4, 6, 3, 'presub_leaky', '', '', 0, (1, 1, 2, 9, 2, 5, 1, 1, 20, 1)),
    ('rs_nch8', 9, 16, 32, 4, 7, 3, 'presub_leaky', '', '', 0, (1, 1, 2, 9, 4, 9, 1, 1, 36, 1)),
    ('rs_B64_off', 64, 16, 16, 7, 7, 3, 'plain', 'conv_wgrad_rsplit=0', '', 0, (1, 1, 1, 9, 1, 16, 1, 1, 64, 1)),
    ('rs_B128_off', 128, 16, 16, 7, 7, 3, 'mask_relu', 'conv_wgrad_rsplit=0', '', 0, (1, 1, 1, 9, 1, 32, 2, 8, 16, 1)),
    ('rs_nch8_off', 9, 16, 32, 4, 7, 3, 'plain', 'conv_wgrad_rsplit=0', '', 0, (1, 1, 2, 9, 1, 3, 1, 1, 12, 1)),
    ('red_64_slots', 64, 16, 16, 6, 8, 1, 'plain', '', '', 0, (1, 1, 1, 1, 1, 16, 1, 1, 64, 1)),
    ('red_68_slots', 68, 16, 16, 6, 8, 1, 'nobias', '', '', 0, (1, 1, 1, 1, 1, 17, 2, 5, 14, 1)),
    ('red_80_slots', 80, 32, 16, 7, 7, 1, 'plain', '', '', 0, (2, 2, 1, 1, 1, 20, 2, 5, 16, 1)),
    ('red_300_slots_k3', 300, 32, 32, 7, 7, 3, 'plain', '', '', 0, (1, 2, 2, 9, 1, 75, 2, 19, 16, 1)),
    ('red_300_slots_k1_direct', 300, 48, 32, 8, 8, 1, 'presub_leaky', '', '', 0, (2, 3, 2, 1, 1, 75, 2, 19, 16, 1)),
    ('ref_cin_24', 9, 24, 16, 7, 7, 3, 'plain', '', '', 1, (0, 0, 0, 0, 0, 0, 0, 0, 0, 0)),
    ('ref_cout_40', 9, 16, 40, 7, 7, 1, 'plain', '', '', 1, (0, 0, 0, 0, 0, 0, 0, 0, 0, 0)),
    ('ref_tiles_3x3_k3', 9, 48, 48, 7, 7, 3, 'plain', '', '', 1, (0, 0, 0, 0, 0, 0, 0, 0, 0, 0)),
    ('ref_no_instance_16_64_k3', 9, 16, 64, 7, 7, 3, 'plain', '', '', 1, (0, 0, 0, 0, 0, 0, 0, 0, 0, 0)),
    ('ref_no_instance_64_16_k3', 9, 64, 16, 7, 7, 3, 'mask_relu', '', '', 1, (0, 0, 0, 0, 0, 0, 0, 0, 0, 0)),
    ('ref_W1', 9, 16, 16, 5, 1, 3, 'plain', '', '', 1, (0, 0, 0, 0, 0, 0, 0, 0, 0, 0)),
    ('ref_65_pixels', 9, 16, 16, 5, 13, 1, 'plain', '', '', 1, (0, 0, 0, 0, 0, 0, 0, 0, 0, 0)),
    ('ref_lds_1x64_32_32_k3', 9, 32, 32, 1, 64, 3, 'plain', '', '', 1, (0, 0, 0, 0, 0, 0, 0, 0, 0, 0)),
    ('ref_lds_8x8_64_64_k1_masked', 9, 64, 64, 8, 8, 1, 'mask_relu', '', '', 1, (0, 0, 0, 0, 0, 0, 0, 0, 0, 0)),
    ('ref_B0', 0, 16, 16, 7, 7, 3, 'plain', '', '', -2, (0, 0, 0, 0, 0, 0, 0, 0, 0, 0)),
    ('ref_x_offset', 9, 16, 16, 7, 7, 3, 'plain', '', 'xoff', -2, (1, 1, 1, 9, 4, 9, 1, 1, 36, 1)),
    ('ref_short_workspace', 9, 16, 16, 7, 7, 3, 'plain', '', 'short_ws', -2, (1, 1, 1, 9, 4, 9, 1, 1, 36, 1)),
]
LN_ROWS = [
    ('ln_C1_B3_P7', 3, 1, 7, 0, 0.0, 0, (1, 16, 1, 1)),
    ('ln_C1_B9_P64', 9, 1, 64, 1, 0.0, 0, (1, 16, 3, 1)),
    ('ln_C15_B5_P49', 5, 15, 49, 1, 0.0, 0, (1, 16, 1, 1)),
    ('ln_C15_B3_P7', 3, 15, 7, 1, 0.1, 0, (1, 16, 1, 1)),
    ('ln_C16_B9_P64', 9, 16, 64, 1, 0.1, 0, (2, 8, 3, 1)),
    ('ln_C16_B5_P49', 5, 16, 49, 0, 0.0, 0, (2, 8, 1, 1)),
    ('ln_C17_B5_P49', 5, 17, 49, 0, 0.0, 0, (1, 32, 1, 1)),
    ('ln_C17_B3_P7', 3, 17, 7, 1, 0.0, 0, (1, 32, 1, 1)),
    ('ln_C31_B9_P64', 9, 31, 64, 1, 0.0, 0, (1, 32, 3, 1)),
    ('ln_C31_B5_P49', 5, 31, 49, 1, 0.1, 0, (1, 32, 1, 1)),
    ('ln_C32_B3_P7', 3, 32, 7, 1, 0.1, 0, (2, 16, 1, 1)),
    ('ln_C32_B9_P64', 9, 32, 64, 0, 0.0, 0, (2, 16, 3, 1)),
    ('ln_C33_B9_P64', 9, 33, 64, 0, 0.0, 0, (1, 64, 3, 1)),
    ('ln_C33_B5_P49', 5, 33, 49, 1, 0.0, 0, (1, 64, 1, 1)),
    ('ln_C47_B3_P7', 3, 47, 7, 1, 0.0, 0, (1, 64, 1, 1)),
    ('ln_C47_B9_P64', 9, 47, 64, 1, 0.1, 0, (1, 64, 3, 1)),
    ('ln_C48_B5_P49', 5, 48, 49, 1, 0.1, 0, (2, 24, 1, 1)),
    ('ln_C48_B3_P7', 3, 48, 7, 0, 0.0, 0, (2, 24, 1, 1)),
    ('ln_C49_B3_P7', 3, 49, 7, 0, 0.0, 0, (1, 64, 1, 1)),
    ('ln_C49_B9_P64', 9, 49, 64, 1, 0.0, 0, (1, 64, 3, 1)),
    ('ln_C63_B5_P49', 5, 63, 49, 1, 0.0, 0, (1, 64, 1, 1)),
    ('ln_C63_B3_P7', 3, 63, 7, 1, 0.1, 0, (1, 64, 1, 1)),
    ('ln_C64_B9_P64', 9, 64, 64, 1, 0.1, 0, (2, 32, 3, 1)),
    ('ln_C64_B5_P49', 5, 64, 49, 0, 0.0, 0, (2, 32, 1, 1)),
    ('ln_C64_relu_300', 300, 64, 49, 1, 0.0, 0, (2, 32, 58, 2)),
    ('ln_cap_k1_C3', 174763, 3, 3, 1, 0.0, 0, (1, 16, 2048, 2)),
    ('ln_cap_k2_C16', 174763, 16, 3, 1, 0.1, 0, (2, 8, 2048, 2)),
    ('ln_ref_C65', 3, 65, 7, 0, 0.0, -2, (0, 0, 0, 0)),
]
# TABLES-END
GR_ROWS = [("gr_ragged", 7, 3 * 49), ("gr_small", 1, 5), ("gr_cap", 3, 1398103), ("gr_empty", 0, 64)]
CTX_ROWS = [(f"ctx_{H}x{W}_k{ks}_B{B}_c{cout}", B, cout, H, W, ks, stride)
            for i, (H, W) in enumerate([(1, 1), (1, 5), (5, 1), (7, 7), (8, 8)])
            for ks, B, cout, stride in ((1, (1, 37)[i % 2], (5, 16)[i % 2], i % 2), (3, (37, 1)[i % 2], (16, 5)[i % 2], 1 - i % 2),
                                        (3, 37, 7, i % 2))]
# jobs: weight gradients of ONE tile shape queued with usf_conv_wgrad_plan_f32 and launched together (names of WG_ROWS); the last
# group mixes pictures whose lds_bytes differ most
JOB_GROUPS = {
    "jobs_T9_1x1": ["t9_1x1_plain_a", "t9_1x1_mask_relu_b", "t9_1x1_presub_leaky_a", "pic_1x64_k3", "rs_B128", "rs_B64_off"],
    "jobs_T9_2x2": ["t9_2x2_plain_b", "t9_2x2_mask_relu_a", "t9_2x2_presub_leaky_b", "t9_2x2_nobias_a"],
    "jobs_T1_2x4": ["t1_2x4_plain_b", "t1_2x4_mask_relu_a", "t1_2x4_presub_leaky_b", "t1_2x4_nobias_a"],
    "jobs_T1_1x1_mixed_lds": ["pic_1x2_k1", "pic_1x64_k1", "pic_8x8_k1", "red_64_slots", "red_68_slots"],
}


def _kn(s):
    return {k: int(v) for k, v in (kv.split("=") for kv in s.split(",") if kv)}


def wg_case(row):
    name, B, cin, cout, H, W, ks, form, kn, fault, rc, expect = row
    c = Case(name=name, B=B, cin=cin, cout=cout, H=H, W=W, ks=ks, form=form, knobs=_kn(kn), fault=fault, rc=rc, expect=tuple(expect))
    c.update(FORMS[form])
    return c


def wg_cases():
    return [wg_case(r) for r in WG_ROWS]


def ln_cases():
    return [Case(name=n, B=B, C=C, P=P, act=act, slope=slope, rc=rc, expect=tuple(e)) for n, B, C, P, act, slope, rc, e in LN_ROWS]


def gr_cases():
    return [Case(name=n, B=B, CP=CP) for n, B, CP in GR_ROWS]


def ctx_cases():
    return [Case(name=n, B=B, cout=co, H=H, W=W, ks=ks, ctx_stride=st) for n, B, co, H, W, ks, st in CTX_ROWS]


def wg_expect(a):
    return (a["kernel"], a["CIT"], a["COT"], a["T"], a["rsplit"], a["blocks"], a["rounds"], a["rows_used"], a["per"],
            a["max_samples_per_wave"]) if a["kernel"] else (0,) * 10


# ---- how the tables were made: the rules, the probes' answers filling in B of regime (b) and every expectation -------------------
def generate_rows(wg_probe, ln_probe):
    """wg_probe(B, cin, cout, H, W, ks, masked, knobs) -> the answer dict of usf_conv_wgrad_variant at CUS compute units and
    BLOCKS_PER_CU; ln_probe(B, C, P) -> that of usf_layernorm_channels_bwd_variant.  Returns (WG_ROWS, LN_ROWS)."""
    rows = []

    def add(name, B, cin, cout, H, W, ks, form, kn="", fault="", rc=0):
        e = wg_expect(wg_probe(max(B, 1), cin, cout, H, W, ks, FORMS[form]["mask"], _kn(kn))) if B > 0 else (0,) * 10
        if rc == 0:
            assert e[0] != 0, name
        rows.append((name, B, cin, cout, H, W, ks, form, kn, fault, rc, e))

    def regime_b(cin, cout, H, W, ks, masked):
        """smallest B with waves of three and of two samples and a ragged last round under conv_wgrad_blocks=2"""
        for B in range(1, 301):
            a = wg_probe(B, cin, cout, H, W, ks, masked, {"conv_wgrad_blocks": 2})
            nsw = a["slots"] // a["rsplit"]
            if a["max_samples_per_wave"] == 3 and B > 2 * nsw and B % nsw:
                return B
        raise AssertionError("no batch up to 300 gives regime (b)")

    def two_regimes(tag, tiles, ks, pics, forms, direct=False):
        k = 0
        for i, (cit, cot) in enumerate(tiles):
            cin, cout = 16 * cit, 16 * cot
            for f, form in enumerate(forms):
                masked = FORMS[form]["mask"]
                for _ in range(len(pics)):                      # the next picture of the cycle this form is served at, on this kernel
                    H, W = pics[k % len(pics)]
                    k += 1
                    if wg_probe(9, cin, cout, H, W, ks, masked, {})["kernel"] == (2 if direct else 1):
                        break
                else:
                    raise AssertionError((tag, cit, cot, form))
                if (i + f) % 2 == 0:
                    add(f"{tag}_{cit}x{cot}_{form}_a", 9, cin, cout, H, W, ks, form)
                else:
                    add(f"{tag}_{cit}x{cot}_{form}_b", regime_b(cin, cout, H, W, ks, masked), cin, cout, H, W, ks, form, "conv_wgrad_blocks=2")

    # every instantiation in both regimes, the forms the forward feeds each
    two_regimes("t9", T9_TILES, 3, [(7, 7), (8, 8), (3, 5), (6, 8), (9, 7), (2, 2), (4, 16)], list(FORMS))
    two_regimes("t1", T1_TILES, 1, [(6, 8), (3, 5), (4, 12), (2, 2), (7, 7), (8, 8), (9, 7), (1, 2), (5, 9)], list(FORMS))
    dp = direct_pictures()
    two_regimes("k1", T1_TILES, 1, [p[0] for p in dp] + [p[1] for p in dp], ["plain", "presub_leaky"], direct=True)
    # (the forms alternate between the regimes, so every instantiation above is in both)
    # pictures of the padded LDS layout, both kernel sizes (masked: kernel 1 stays on the LDS-staged kernel above 48 pixels)
    for H, W in PICTURES:
        for ks in (3, 1):
            add(f"pic_{H}x{W}_k{ks}", 9, 16, 16, H, W, ks, "mask_relu")
    add("pic_6x8_k1_unmasked_48_pixels", 9, 32, 16, 6, 8, 1, "presub_leaky")        # H W = 48: the LDS-staged kernel, not the direct one
    # rsplit: both sides of each threshold; conv_wgrad_rsplit=0 for one of each
    for B in (64, 65, 128, 129):
        add(f"rs_B{B}", B, 16, 16, 7, 7, 3, "plain")
    for nch, (H, W) in NCH_PICTURES.items():
        add(f"rs_nch{nch}", 9, 16, 32, H, W, 3, "presub_leaky")
    add("rs_B64_off", 64, 16, 16, 7, 7, 3, "plain", "conv_wgrad_rsplit=0")
    add("rs_B128_off", 128, 16, 16, 7, 7, 3, "mask_relu", "conv_wgrad_rsplit=0")
    add("rs_nch8_off", 9, 16, 32, 4, 7, 3, "plain", "conv_wgrad_rsplit=0")
    # the sum over the slots: 64 slots (one round), 68 (two, ragged last row), 80 (two, even rows), the largest at B = 300
    add("red_64_slots", 64, 16, 16, 6, 8, 1, "plain")
    add("red_68_slots", 68, 16, 16, 6, 8, 1, "nobias")
    add("red_80_slots", 80, 32, 16, 7, 7, 1, "plain")
    add("red_300_slots_k3", 300, 32, 32, 7, 7, 3, "plain")
    add("red_300_slots_k1_direct", 300, 48, 32, 8, 8, 1, "presub_leaky")
    # refusals and argument checks
    add("ref_cin_24", 9, 24, 16, 7, 7, 3, "plain", rc=1)
    add("ref_cout_40", 9, 16, 40, 7, 7, 1, "plain", rc=1)
    add("ref_tiles_3x3_k3", 9, 48, 48, 7, 7, 3, "plain", rc=1)
    add("ref_no_instance_16_64_k3", 9, 16, 64, 7, 7, 3, "plain", rc=1)          # CIT * COT = 4 passes the register rule; no <1,4,9>
    add("ref_no_instance_64_16_k3", 9, 64, 16, 7, 7, 3, "mask_relu", rc=1)
    add("ref_W1", 9, 16, 16, 5, 1, 3, "plain", rc=1)
    add("ref_65_pixels", 9, 16, 16, 5, 13, 1, "plain", rc=1)
    add("ref_lds_1x64_32_32_k3", 9, 32, 32, 1, 64, 3, "plain", rc=1)
    add("ref_lds_8x8_64_64_k1_masked", 9, 64, 64, 8, 8, 1, "mask_relu", rc=1)      # (its unmasked form runs on the direct kernel)
    add("ref_B0", 0, 16, 16, 7, 7, 3, "plain", rc=-2)
    add("ref_x_offset", 9, 16, 16, 7, 7, 3, "plain", fault="xoff", rc=-2)
    add("ref_short_workspace", 9, 16, 16, 7, 7, 3, "plain", fault="short_ws", rc=-2)

    ln = []

    def addl(name, B, C, P, act, slope, rc=0):
        a = ln_probe(B, C, P)
        ln.append((name, B, C, P, act, slope, rc, (a["kernel"], a["width"], a["blocks"], a["rounds"])))

    acts = [(NONE, 0.0), (LEAKY, 0.0), (LEAKY, 0.1)]
    sizes = [(3, 7), (5, 49), (9, 64)]              # B P = 21 (< 32), 245 (no multiple of 32), 576 (three blocks, the last ragged)
    for i, C in enumerate((1, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64)):
        for j in range(2):
            B, P = sizes[(i + 2 * j + i // 3) % 3]
            addl(f"ln_C{C}_B{B}_P{P}", B, C, P, *acts[(i + j) % 3])
    addl("ln_C64_relu_300", 300, 64, 49, LEAKY, 0.0)                        # 58 blocks: two reduction rounds
    addl("ln_cap_k1_C3", 174763, 3, 3, LEAKY, 0.0)                          # B P = 2048 * 256 + 1: the grid-stride loop
    addl("ln_cap_k2_C16", 174763, 16, 3, LEAKY, 0.1)
    addl("ln_ref_C65", 3, 65, 7, NONE, 0.0, rc=-2)
    return rows, ln


# ---- data: everything from seeded CPU generators -----------------------------------------------------------------------------
def _rng(*key):
    return np.random.default_rng(int.from_bytes("|".join(map(str, key)).encode(), "little") % (1 << 63))


def _normal(r, shape, zeros=0.1):
    v = r.standard_normal(shape, dtype=np.float32)
    if zeros:
        v[r.random(shape, dtype=np.float32) < zeros] = 0.0
    return v


def wg_data(c):
    """x [B, cin, H, W] (exact zeros; under pre_sub also elements equal to their channel's pre_sub), dy [B, cout, H, W] (channel 1
    of every 16 scaled by 2^-24: small elements a max-norm bound does not see), in_mul [cin H W] of 0 / 1, pre_sub [cin]"""
    r = _rng("wg", c.cin, c.cout, c.H, c.W, c.ks, c.form, c.B)
    B = max(c.B, 1)
    d = Case()
    x = _normal(r, (B, c.cin, c.H, c.W))
    dy = _normal(r, (B, c.cout, c.H, c.W), zeros=0.02)
    dy[:, 1::16] *= np.float32(2.0 ** -24)
    d.pre_sub = d.in_mul = None
    if c.pre_sub:
        ps = r.standard_normal(c.cin, dtype=np.float32)
        hit = r.random(x.shape, dtype=np.float32) < 0.05
        x = np.where(hit, np.broadcast_to(ps.reshape(1, -1, 1, 1), x.shape), x)
        d.pre_sub = torch.from_numpy(ps)
    if c.mask:
        d.in_mul = torch.from_numpy((r.random(c.cin * c.H * c.W) < 0.5).astype(np.float32))
    d.x, d.dy = torch.from_numpy(np.ascontiguousarray(x)), torch.from_numpy(dy)
    return d


def ln_data(c):
    r = _rng("ln", c.B, c.C, c.P, c.act, c.slope)
    d = Case()
    d.x = torch.from_numpy(_normal(r, (c.B, c.C, c.P)))
    d.dy = torch.from_numpy(_normal(r, (c.B, c.C, c.P), zeros=0.02))
    d.gamma = torch.from_numpy((1 + 0.3 * r.standard_normal(c.C)).astype(np.float32))
    d.eps = 1e-5
    return d


def gr_data(c):
    r = _rng("gr", c.B, c.CP)
    d = Case()
    d.dy = torch.from_numpy(_normal(r, (c.B, c.CP)))
    vg = 3 * r.standard_normal((c.B, 2, c.CP), dtype=np.float32)
    vg[:, 1].reshape(-1)[:4] = [0.0, 30.0, -30.0, 100.0][:min(4, vg[:, 1].size)]          # gates where the sigmoid saturates
    d.vg = torch.from_numpy(vg)
    return d


def ctx_data(c):
    r = _rng("ctx", c.B, c.cout, c.H, c.W, c.ks, c.ctx_stride)
    d = Case()
    d.dy = torch.from_numpy(_normal(r, (c.B, c.cout, c.H, c.W)))
    d.ctx = torch.from_numpy(r.standard_normal(c.B if c.ctx_stride else 1, dtype=np.float32))
    return d


# ---- the statements: (outputs, magnitudes) in `dtype` on the operands' device -----------------------------------------------------
def _seq_sum(terms, n):
    """strictly sequential accumulation of terms(i), i < n, in the terms' dtype"""
    acc = terms(0)
    for i in range(1, n):
        acc = acc + terms(i)
    return acc


def wg_xin(c, d, dtype):
    """(xin, |xin| bound): in_act(x - pre_sub) * in_mul and the same with every term replaced by its magnitude"""
    x = d.x.to(dtype)
    a = x.abs()
    if d.pre_sub is not None:
        ps = d.pre_sub.to(dtype).view(1, -1, 1, 1)
        x, a = x - ps, a + ps.abs()
    if c.act == LEAKY:
        x, a = torch.where(x > 0, x, x * c.slope), torch.where(x > 0, a, a * abs(c.slope))
    if d.in_mul is not None:
        m = d.in_mul.to(dtype).view(1, c.cin, c.H, c.W)
        x, a = x * m, a * m.abs()
    return x, a


def wg_forward(c, d, dtype, mode="einsum", samples=None):
    """dict(dW [cout, cin, ks, ks], db [cout], A_dW, A_db); mode "seq": one product per sample, added in sample order; samples:
    the sample indices that enter (a planted defect drops or repeats one)"""
    xin, axin = wg_xin(c, d, dtype)
    dy = d.dy.to(dtype)
    if samples is not None:
        idx = torch.as_tensor(samples, device=xin.device)
        xin, axin, dy = xin[idx], axin[idx], dy[idx]
    B = xin.shape[0]
    cols, acols = F.unfold(xin, c.ks, padding=c.ks // 2), F.unfold(axin, c.ks, padding=c.ks // 2)       # [B, cin ks ks, HW]
    dyf = dy.flatten(2)
    shape = (c.cout, c.cin, c.ks, c.ks)
    if mode == "einsum":
        dW = torch.einsum("bop,bkp->ok", dyf, cols)
        db = dyf.sum(dim=(0, 2))
    else:
        dW = _seq_sum(lambda b: dyf[b] @ cols[b].T, B)
        db = _seq_sum(lambda b: dyf[b].sum(1), B)
    return Case(dW=dW.reshape(shape), db=db, A_dW=torch.einsum("bop,bkp->ok", dyf.abs(), acols).reshape(shape), A_db=dyf.abs().sum(dim=(0, 2)))


def ln_forward(c, d, dtype, mode="einsum", defect=None):
    """dict(dx, dgamma, dbeta, A_*): the header's formulas; the magnitudes bound every subtraction by the sum of its terms"""
    x, dy, gam = d.x.to(dtype), d.dy.to(dtype), d.gamma.to(dtype).view(1, -1, 1)
    a = torch.where(x > 0, x, x * c.slope) if c.act == LEAKY else x
    mean = (a[:, :-1].sum(1, keepdim=True) / c.C) if defect == "channel_left_out" else a.mean(1, keepdim=True)
    t = a - mean
    rden = 1 / torch.sqrt((t * t).mean(1, keepdim=True) + d.eps)
    xh = t * rden
    axh = (a.abs() + a.abs().mean(1, keepdim=True)) * rden
    g = dy * gam
    m1, m2 = g.mean(1, keepdim=True), (g * xh).mean(1, keepdim=True)
    da = (g - m1 - xh * m2) * rden
    ada = (g.abs() + g.abs().mean(1, keepdim=True) + axh * (g.abs() * axh).mean(1, keepdim=True)) * rden
    if c.act == LEAKY:
        gate = torch.where((x >= 0) if defect == "gate_at_zero" else (x > 0), torch.ones_like(x), torch.full_like(x, c.slope))
        da, ada = da * gate, ada * gate.abs()
    if mode == "einsum":
        dg, dbt = (dy * xh).sum(dim=(0, 2)), dy.sum(dim=(0, 2))
    else:
        n = c.B if c.B <= 512 else 512                  # sample by sample; the two large rows in 512 slices of the batch
        sl = [slice(i * c.B // n, (i + 1) * c.B // n) for i in range(n)]
        dg = _seq_sum(lambda i: (dy[sl[i]] * xh[sl[i]]).sum(dim=(0, 2)), n)
        dbt = _seq_sum(lambda i: dy[sl[i]].sum(dim=(0, 2)), n)
    return Case(dx=da, dgamma=dg, dbeta=dbt, A_dx=ada, A_dgamma=(dy.abs() * axh).sum(dim=(0, 2)), A_dbeta=dy.abs().sum(dim=(0, 2)))


def gr_forward(c, d, dtype):
    dy, vg = d.dy.to(dtype), d.vg.to(dtype)
    val, gate = vg[:, 0], vg[:, 1]
    s = 1 / (1 + torch.exp(-gate))
    dvg = torch.stack([dy * s, dy * val * (s * (1 - s))], 1)
    return Case(dvg=dvg, A_dvg=torch.stack([dy.abs() * s, dy.abs() * val.abs() * (s * (1 + s))], 1))


def ctx_forward(c, d, dtype, mode="einsum"):
    """dw_ctx [cout, ks ks]: tap t sums dy over the pixels whose tap t lands inside the picture, weighted by the sample's context"""
    dy = d.dy.to(dtype)
    ctx = (d.ctx if c.ctx_stride else d.ctx.expand(c.B)).to(dtype)
    ones = torch.ones(1, 1, c.H, c.W, dtype=dtype, device=dy.device)
    inside = F.unfold(ones, c.ks, padding=c.ks // 2)[0]                                    # [ks ks, HW]: 1 where the tap is inside
    per = lambda v: torch.einsum("bop,tp->bot", v.flatten(2), inside)                      # [B, cout, taps]
    if mode == "einsum":
        dw = torch.einsum("b,bot->ot", ctx, per(dy))
    else:
        pd = per(dy)
        dw = _seq_sum(lambda b: ctx[b] * pd[b], c.B)
    return Case(dw=dw, A_dw=torch.einsum("b,bot->ot", ctx.abs(), per(dy.abs())))


# ---- the checker -----------------------------------------------------------------------------------------------------------------
def guarded(n, device="cpu", lead=0):
    """GUARD sentinels | n floats (sentinels too: an element the launch leaves is found) | GUARD sentinels"""
    return torch.full((lead + GUARD + n + GUARD,), sentinel(), dtype=torch.float32, device=device)[lead:]


def untouched(buf):
    return bool((bits(buf) == SENTINEL_BITS).all())


def ratio(got, ref64, A64):
    """worst |got - ref64| / (U * A) over every element (0 / 0 counts as 0, x / 0 as inf)"""
    err = (got.double() - ref64).abs()
    return torch.where(err == 0, torch.zeros_like(err), err / (U * A64)).max().item() if err.numel() else 0.0


def check(what, buf, ref64, A64, family, maxnorm=True, lo=GUARD, front=True, behind=True):
    """every finding of one output's guarded buffer against the fp64 statement; [] = it passes.  The per-element bound is
    MARGIN * K[family] * U * A, the suite's earlier max-norm bound stays next to it.  lo / front / behind: the output starts at
    float `lo` of the buffer and has the front / rear sentinels next to it (two outputs that share one guarded buffer)"""
    n = ref64.numel()
    out = []
    s = torch.tensor([SENTINEL_BITS], dtype=torch.int32, device=buf.device)
    if front and not bool((bits(buf[:lo]) == s).all()):
        out.append(f"written in front of {what}")
    if behind and not bool((bits(buf[lo + n:]) == s).all()):
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
        idx = np.unravel_index(i, tuple(got.shape))
        out.append(f"{int(over.sum())} elements of {what} over {bound:.1f} U A; worst at {idx}: got {got.flatten()[i].item()!r}, fp64 "
                   f"{ref64.flatten()[i].item()!r}, A {A64.flatten()[i].item()!r}")
    if maxnorm and not maxnorm_ok(got, ref64, family):
        out.append(f"max-norm bound of {what}: {err.max().item():.3e} > {MAXNORM[family]} * {ref64.abs().max().item():.3e}")
    return out


def maxnorm_ok(got, ref64, family):
    """the bound the suite held these kernels to before: max |err| <= tol * max |ref|"""
    if not ref64.numel():
        return True
    return (got.double() - ref64).abs().max().item() <= MAXNORM[family] * max(ref64.abs().max().item(), 1e-30)
