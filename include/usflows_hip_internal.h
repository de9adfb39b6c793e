/*
 * usflows_hip_internal.h -- the rest of libusflows_hip.so's C exports: the plumbing of the Python engine (usflows_amd) that
 * happens to cross the C boundary.  Every backward, weight-gradient and job-queue entry point of the training path, the
 * SophiaG and Adam optimizers and the gradient clip, which kernel variant a descriptor selects, and the measurement / tuning aids.
 *
 * NO STABILITY PROMISE: anything here may change in any release.  Such a change bumps USF_INTERNAL_VERSION, never
 * USF_ABI_VERSION, which covers usflows_hip.h alone.  A binding that mirrors this file checks usf_internal_version() next
 * to usf_abi_version().  The boundary contract of usflows_hip.h holds for every entry point here.
 */
#ifndef USFLOWS_HIP_INTERNAL_H
#define USFLOWS_HIP_INTERNAL_H

#include "usflows_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define USF_INTERNAL_VERSION 6

/* USF_INTERNAL_VERSION of the header the library was built from (host only, launches nothing). */
int usf_internal_version(void);

/*
 * Training-path fields of the public descriptors (declared in usflows_hip.h, where they keep their place in the layout).
 *
 * usf_linear_desc::A_planes_out, ldp_out, planes_out_stride:
 *   Optional side output (ABI 32): the three row-major bf16 planes of the INPUT A (A == p1 + p2 + p3 exactly, the
 *   split the bf16x3 kernel makes of its operand anyway), plane p at A_planes_out + p * planes_out_stride elements,
 *   each [ceil32(M), ldp_out] bf16 with ldp_out >= ceil32(K), ldp_out % 8 == 0; rows [M, ceil32(M)) are NOT written by the
 *   bf16x3 kernels (the caller's buffer holds zeros there: usf_wgrad_planes_f32 sums over them), columns [K, ceil32(K)) receive
 *   finite padding.  Where another kernel serves the product (small M, no W_split), the planes come from a usf_split_planes_f32
 *   pass, which writes the whole [ceil32(M), ldp_out] image: zeros in rows [M, ceil32(M)) and in columns [K, ldp_out).  Either
 *   way a buffer that held zeros in the padding rows still does.  This is the operand layout of usf_wgrad_planes_f32: the
 *   data-gradient / forward GEMM of a layer hands the weight gradient of the same layer its operand already split
 *   (flows.py:196-203: loss.backward() through every F.linear of the flow).  Not with pre_div / pre_sub.
 *
 * usf_coupling_desc::hidden_out, ld_hidden_out:
 *   Optional (ABI 32): hidden_out[l] [M, ld_hidden_out] receives the activations of hidden layer l (after the
 *   nonlinearity; the padded width, zeros in the padding) -- what the backward pass of the training step otherwise computes a
 *   second time (two GEMMs per coupling layer; flows.py:196-203).  Only the bf16x3 kernel stores them (its eligibility rule
 *   in usflows_hip.h): a descriptor that sets hidden_out and is served by another kernel is rejected.  ld_hidden_out % 4 == 0,
 *   16-byte aligned bases.
 *
 * usf_coupling_desc::gate, ld_gate:
 *   act == USF_ACT_GATE (ABI 32; bf16x3 kernel only, no context): hidden layer l's pre-activation is not passed through
 *   the nonlinearity but multiplied by (gate[l][m, j] > 0 ? 1 : slope), gate[l] [M, ld_gate] -- the conditioner's BACKWARD
 *   pass on the same kernel: with the transposed weights (W_in = W_out^T, W_hid reversed and transposed, W_out = W_in^T),
 *   zero biases, the column segments swapped (pass <-> trans) and gate[l] = the forward's saved activation of hidden layer
 *   n_hidden - 1 - l, the launch computes  g[:, pass] += sign * d_h1 W_in  from g[:, trans]  and hidden_out receives the
 *   gradients at the hidden activations (d_h of the last hidden layer first): what autograd derives for the MLP of
 *   MaskedCoupling (transforms.py:277-306, networks.py:739-751) in three GEMM launches + gates.
 *
 * usf_pack_planes_desc::row_weight, loc, scale, grad_base:
 *   optional, src_cols > 0 only: the source is transformed on the way in -- the head of the TRAINING backward pass,
 *   src = the latent z and the planes receive  g[m, c] = row_weight[m] * d/dz base_c(z[m, c])  (usf_base_logprob_grad_f32's
 *   formulas for USF_BASE_LAPLACE / USF_BASE_NORMAL with loc / scale [src_cols]; grad_base = 1 + base id, 0 = plain copy)
 *
 * usf_coupling_planes_desc::hidden_out, gate:
 *   Training (ABI 33; USF_PLANES_BF16X3, n_hidden <= 2).  Planes buffers with 8 blocks per panel (hidden width 256):
 *     hidden_out[l] (optional, all n_hidden or none): receives the activations of hidden layer l -- the lane-local splits
 *       the kernel makes anyway, i.e. the operands of the conditioner's weight gradients (usf_wgrad_blocked_f32) and the
 *       gates of the backward launch.
 *     act == USF_ACT_GATE (needs hidden_out and gate[l] for every layer): the launch runs the conditioner's data-gradient
 *       chain -- the caller passes the transposed weight images in reverse order, zero biases and swaps the block ranges:
 *       z = the gradient buffer, g[:, pass] += sign * MLP^T(g[:, trans]); layer l's nonlinearity is leaky_relu_backward
 *       from the saved activations gate[l] (v * (h > 0 ? 1 : slope); only plane 0 of gate[l] is read) and hidden_out[l]
 *       receives the gated values (the gradients at the pre-activations of forward hidden layer n_hidden - 1 - l).
 *   Replaces autograd's backward of MaskedCoupling + its conditioner (transforms.py:277-306, networks.py:739-751) under
 *   Flow.fit (flows.py:196-203) at batches of thousands of rows.
 *
 * usf_sizeof_desc(kind) also reports sizeof(usf_mt_chunk|usf_grad_job|usf_psum_job) for kind 8|11|12 and
 * sizeof(usf_gated_norm_bwd_desc|usf_wgrad_job|usf_wreduce_job|usf_wplanes_job) for kind 13|14|15|16 and
 * sizeof(usf_adam_chunk|usf_grad_chunk|usf_conv_variant_query|usf_conv_variant) for kind 17|18|19|20 and
 * sizeof(usf_conv_wgrad_query|usf_conv_wgrad_info|usf_ln_bwd_info) for kind 21|22|23 and
 * sizeof(usf_conv_band_query|usf_conv_band_info) for kind 27|28 and
 * sizeof(usf_conv_wgrad_band_query|usf_conv_wgrad_band_info) for kind 29|30.
 */

/*
 * Which kernel family / instantiation usf_linear_f32 would launch for this descriptor (nothing is launched):
 *   1000                          small-batch kernel (M <= 768)
 *   2000 + 100 TM + 10 TN + WM    exact-f32 MFMA tile
 *   3000 + 100 TN + 10 WM + NB    bf16x3 tile (TN x 32 columns, WM waves x 32 rows, NB weight buffers)
 * 0 for a descriptor with empty extents.  The parity tests use it to prove that every instantiation the BASELINE
 * configurations select is compared with the reference arithmetic (tests/test_configs_gpu.py).
 */
int usf_linear_variant(const usf_linear_desc* d);

/* which kernel usf_coupling_additive_f32 launches for this descriptor (nothing is launched, no pointer is dereferenced):
 * 3 the tiny-layer kernel (M <= 256, segments and hidden widths <= 64, the layer's images in 64 KB of LDS: usf_coupling_tiny.hip),
 * 2 the bf16x3 kernel, 1 the exact-f32 MFMA kernel, 0 for a NULL descriptor */
int usf_coupling_variant(const usf_coupling_desc* d);

/*
 * The backward of usf_radial_logprob_f32 (usflows_hip.h), same operands:
 * usf_radial_logprob_grad_f32: from g_lp [M] (gradient at logp) and the saved r:
 *     g[m,d]   = g_lp[m] * dlogp/dr * dr/dz[m,d]   (0 for D <= d < ldg; ATen's norm backward: p = 1 sign(t), p = 2 t / r,
 *                                                   p = inf sign(t) / (number of d with |t| == r) where |t| == r: tied
 *                                                   maxima share the gradient evenly, as x.norm(p=inf) does)
 *     r == 0 (z == loc exactly): log r = -inf and (D - 1) / r = inf enter the row as they do in the reference
 *     (distributions.py:506-549): logp is +-inf or NaN depending on the norm distribution and the row of g is NaN (p = 2: t / r
 *     is taken as 0) -- nothing is clamped.
 *     d_loc[d] = -sum_m g[m,d];   d_a / d_b / d_logits [K] = gradients of the STORED parameters (chain rule through softplus)
 * each output pointer but g is optional.  z == NULL (both entry points): the radii are GIVEN -- the forward reads r_out as its
 * input, the backward writes g [M] = the gradient at r (d_loc must be NULL): the finishing formula alone, for callers whose own
 * tail kernel reduces the radius (the flat training path).  Partial sums are added in a fixed order (bit-reproducible).  workspace: at least
 * usf_radial_logprob_grad_workspace(M, D) bytes, 8-byte aligned.
 */
int64_t usf_radial_logprob_grad_workspace(int64_t M, int64_t D);
int usf_radial_logprob_grad_f32(const float* z, int64_t ldz, const float* r, const float* g_lp, int64_t M, int64_t D, int32_t p_id,
                                const float* loc, int32_t norm, int32_t K, const float* par_a, const float* par_b,
                                const float* logits, float* g, int64_t ldg, float* d_loc, float* d_a, float* d_b, float* d_logits,
                                void* workspace, int64_t workspace_bytes, usf_stream_t stream);

/*
 * usf_radial_sample_norm_f32 (an ADDED entry point: every declaration of internal version 4 is unchanged, so the number stays;
 * a binding that declares it refuses a library without it when it resolves the symbol): RadialDistribution.sample (distributions.py:474-499) in ONE launch -- the
 * radius r[m] ~ norm_distribution AND z[m, :D] = loc + r[m] * u, u uniform on the unit Lp sphere -- as a pure function of
 * (seed, offset, m + row_offset, parameters): the same rows for any split of a draw over launches or ranks, no host read-back.
 *   norm, K, par_a, par_b, logits: exactly as for usf_radial_logprob_f32 (usflows_hip.h): stored parameters, softplus applied
 *     inside unless USF_NORM_RAW_PARAMS, 1 <= K <= 64, USF_NORM_CHI raw only, par_b NULL for USF_NORM_HALFNORMAL, logits
 *     required for K > 1.
 *   r_out [M], optional: receives every row's radius.  z == NULL: the radii only (r_out required; D, loc, p_id ignored).
 * The radius is computed in fp64 and rounded to fp32 once.  With ph(t) = philox4x32_10(counter m + row_offset, stream
 * offset ^ 0x85ebca6b ^ (t << 32), key seed) = words w0..w3, u(w) = (w + 1/2) 2^-32 and n = sqrt(-2 ln u(w1)) cos(2 pi u(w2)):
 *   component k = #{j : C_j <= u(w0 of ph(0)) C_{K-1}} capped at K - 1, C_j = sum_{i <= j} exp(l_i - max l) in index order
 *   LogNormal  r = exp(mu + sigma n)  [ph(0)]       HalfNormal  r = sigma |n|       Weibull  r = lambda (-ln u(w1))^(1/k)
 *   Gamma(a, rate b): Marsaglia-Tsang with a' = a < 1 ? a + 1 : a, d = a' - 1/3, c = 1 / sqrt(9 d); attempt t = 0 .. 31 takes
 *     w1..w3 of ph(t), v = (1 + c n)^3, accepts when v > 0 and ln u(w3) < n^2 / 2 + d - d v + d ln v, then g = d v; the loop
 *     bound is a compile-time constant and g = d when no attempt accepted (the kernel cannot spin); a < 1: g *=
 *     u(w0 of ph(0xFFFF))^(1/a);  r = g / b
 *   Chi(nu, s): that draw with shape nu / 2, r = s sqrt(2 g)
 *   r is clamped from below to the smallest normal fp32 (as torch's Gamma.rsample).
 * The direction uses usf_radial_sample_f32's counters, streams and arithmetic unchanged: z is bit for bit what that entry
 * point writes when handed r_out.  Columns [D, ldz) are not written.  Returns -2 (sizes, ids, K) / -1 (null pointer) with
 * usf_last_error set before anything is launched.
 */
int usf_radial_sample_norm_f32(float* z, int64_t ldz, int64_t M, int64_t D, int32_t p_id, const float* loc,
                               int32_t norm, int32_t K, const float* par_a, const float* par_b, const float* logits,
                               float* r_out, uint64_t seed, uint64_t offset, int64_t row_offset, usf_stream_t stream);

/*
 * usf_coupling_planes_ctx (internal version 3): usf_coupling_planes (usflows_hip.h) whose conditioner is a ConditionalDenseNN
 * with context_dim == 1 (networks.py:739-751: layers[1](context) is added to the first layer's pre-activation).  The first
 * layer's accumulators start at
 *     b_in[h] + b_ctx[h] + ctx[m * ctx_stride] * w_ctx[h]                  (row m, hidden unit h)
 * instead of b_in[h] -- a rank-1 term: no matrix instruction, no LDS, nothing in the K loops.  ctx: fp32, one value per row
 * (ctx_stride == 1, M values) or one for all rows (ctx_stride == 0); nothing is read outside ctx, and a launch with a context
 * leaves the rows of z's last panel beyond M as they are (usf_coupling_planes rewrites them from their own values).
 * w_ctx / b_ctx: [256] fp32 (layers[1].weight[:, 0] / layers[1].bias), zero beyond the real width, 16-byte aligned.
 * Inference and the training forward (hidden_out) in both plane formats, n_hidden 1..3 as usf_coupling_planes serves them;
 * USF_ACT_GATE with a context is rejected (the backward chain has no context term: the context enters no data gradient).
 * ctx == NULL: exactly usf_coupling_planes (same kernels, same bits).  Arguments are validated before any launch.
 *
 * Inside an op list (usf_run_ops): the public usf_op union does not grow.  A USF_OP_CALL op with fn ==
 * USF_FN_COUPLING_PLANES_CTX and n_args == 4 carries (ctx, ctx_stride, w_ctx, b_ctx) as its words a[0..3] and applies to the
 * USF_OP_COUPLING_PLANES op that must follow it directly: the pair is ONE usf_coupling_planes_ctx launch.  (Function ids from
 * USF_FN_INTERNAL_BASE on are internal; usflows_hip.h's run 1..12 and must stay below it: the library asserts that at compile
 * time.)  A list that ends behind the prefix op, or whose next op is of another kind, is rejected.
 */
#define USF_FN_INTERNAL_BASE 64
#define USF_FN_COUPLING_PLANES_CTX 64
int usf_coupling_planes_ctx(const usf_coupling_planes_desc* d, const float* ctx, int64_t ctx_stride, const float* w_ctx,
                            const float* b_ctx, usf_stream_t stream);

/*
 * usf_gemm_planes_side / usf_coupling_planes_side (ADDED entry points: every declaration of internal version 6 is unchanged, so
 * the number stays; a binding that declares them refuses a library without them when it resolves the symbols).
 * The transformed half of an affine layer's output has one reader in an inference plan: the output phase of the fused coupling
 * behind it, which wants it as fp32 (the residual of fma(sign, acc, residual)).  The pair hands it over as fp32 beside the planes:
 *   side buffer: ceil(M / 16) panels x side_kbn blocks x 2 KiB, 16-byte aligned, below 4 GiB (32-bit offsets).  Chunk (panel p,
 *     block j) lies at (p * side_kbn + j) * 2048; lane L = 16 g + j' holds 32 bytes at L * 32: the fp32 values of the 8 slots
 *     that lane holds in a planes chunk (usflows_hip.h), in slot order.
 *   usf_gemm_planes_side: usf_gemm_planes_bf16x3 with planes output and no residual, whose output blocks [side_kb0, side_kb0 +
 *     side_kbn) (counted from c_kb0, inside [0, c_kbn)) go to the side buffer (block side_kb0 + j to chunk j) and NOT to
 *     C_planes -- except the blocks of [both_kb0, both_kb0 + both_kbn), a sub-range of the side range (both_kbn == 0: none),
 *     which are written both ways: the block that holds conditioning and transformed features.  The other blocks are written
 *     as planes, as always.  USF_PLANES_BF16X3: the side value is the accumulator -- the float whose exact three-way split the
 *     planes would hold (exact for every value whose last bit is worth 2^-133 or more; an accumulator of -0, whose planes sum
 *     to +0, arrives as -0).  USF_PLANES_F16X2: the side value is
 *     the sum of the two fp16 planes the value would have been stored as, and the range guard looks at it as always.
 *   usf_coupling_planes_side: usf_coupling_planes (inference: no context, no hidden_out, no USF_ACT_GATE) whose output phase
 *     reads the residual of transformed block nt from chunk nt of the side buffer (side_nkb must equal nk_t) instead of
 *     rebuilding it from z's planes.  It reads the conditioning blocks of z and writes its transformed blocks as always -- the
 *     same bytes as usf_coupling_planes on a z whose transformed blocks hold the planes of the side values; what those blocks
 *     held before is not read.
 * Returns -1 (null pointer), -2 (alignment, block ranges, a descriptor the side form does not serve), -3 (a side buffer of
 * 4 GiB or more) with usf_last_error set before anything is launched.
 *
 * Inside an op list the public usf_op union does not grow: a USF_OP_CALL op with fn == USF_FN_GEMM_PLANES_SIDE and n_args == 5
 * carries (side, side_kb0, side_kbn, both_kb0, both_kbn) and applies to the USF_OP_GEMM_PLANES op that must follow it directly;
 * one with fn == USF_FN_COUPLING_PLANES_SIDE and n_args == 2 carries (side, side_nkb) and applies to the USF_OP_COUPLING_PLANES
 * op that must follow it directly.  Each pair is ONE launch.  A list that ends behind a prefix op, or whose next op is of
 * another kind, is rejected.
 */
#define USF_FN_GEMM_PLANES_SIDE 66
#define USF_FN_COUPLING_PLANES_SIDE 67
int usf_gemm_planes_side(const usf_gemm_planes_desc* d, void* side, int64_t side_kb0, int64_t side_kbn, int64_t both_kb0,
                         int64_t both_kbn, usf_stream_t stream);
int usf_coupling_planes_side(const usf_coupling_planes_desc* d, const void* side, int64_t side_nkb, usf_stream_t stream);

/*
 * usf_coupling_additive_vctx_f32 (internal version 4): usf_coupling_additive_f32 (usflows_hip.h) whose conditioner is a
 * ConditionalDenseNN with 1 <= context_dim <= USF_VCTX_MAX (networks.py:681-751: h = layers[0](x) + layers[1](context)).
 * The first hidden layer's pre-activation becomes
 *     v + ( b_ctx[h] + sum_{c < ctx_dim} ctx[m * ld_ctx + c] * W_ctx_t[c * ldw_ctx + h] )           (row m, hidden unit h)
 * -- a rank-ctx_dim term summed in fp32 over c in ascending order and added as ONE value: no matrix instruction, nothing in the
 * K loops.  It runs in all three kernel families of usf_coupling_additive_f32 (the exact-f32, the bf16x3 and the tiny-layer
 * kernel), as instantiations of their own: the descriptors without this entry's context run the kernels they always ran.
 *   ctx       fp32 rows of ld_ctx floats, 16-byte aligned; ld_ctx a multiple of 4 and >= round_up(ctx_dim, 4) (M rows), or
 *             ld_ctx == 0: ONE row for all rows.  PADDING CONTRACT: only the columns [0, ctx_dim) enter the arithmetic.  A
 *             kernel may LOAD the padding columns [ctx_dim, round_up(ctx_dim, 4)) of a row (they must be readable memory, also
 *             with ld_ctx == 0) but never multiplies them in: whatever they hold -- NaN included -- leaves the output unchanged.
 *   W_ctx_t   the context weights TRANSPOSED, layers[1].weight^T as [ctx_dim, ldw_ctx] fp32 rows: a lane's four consecutive
 *             hidden units are one 16-byte load per context column.  16-byte aligned, ldw_ctx a multiple of 4 and >= the
 *             padded hidden width the kernel runs at (usf_coupling_padded_width(widest hidden layer); the tiny-layer kernel
 *             reads hidden[0] columns only), zeros beyond the real width.
 *   b_ctx     layers[1].bias, fp32 of that padded width, zeros beyond the real width, 16-byte aligned.
 * d->context, d->W_ctx and d->b_ctx must be NULL.  USF_ACT_GATE with a context is rejected (the backward chain has no context
 * term: the context enters no data gradient); hidden_out (the training forward) is served where usf_coupling_additive_f32
 * serves it.  ctx == NULL: exactly usf_coupling_additive_f32 (same kernels, same bits).  Every argument is validated before
 * any launch; an error launches nothing.
 *
 * usf_coupling_additive_vctx_variant: which kernel the entry point launches for the descriptor with a context of ctx_dim
 * columns (3 / 2 / 1 / 0 as usf_coupling_variant; nothing is launched, no pointer is dereferenced).  The tiny-layer kernel
 * keeps the rows' context ([32, ctx_dim]) and W_ctx_t ([ctx_dim, hidden[0]]) in LDS: a layer whose images no longer fit
 * the 64 KB with them is served by the MFMA kernels (whose alignment rules then apply) -- it selects another kernel, it does
 * not fail.  ctx_dim == 0: usf_coupling_variant.
 *
 * Inside an op list: a USF_OP_CALL op with fn == USF_FN_COUPLING_VCTX and n_args == 6 carries (ctx, ld_ctx, ctx_dim, W_ctx_t,
 * ldw_ctx, b_ctx) as its words a[0..5] and applies to the USF_OP_COUPLING op that must follow it directly: the pair is ONE
 * usf_coupling_additive_vctx_f32 launch.  A list that ends behind the prefix op, or whose next op is of another kind, is
 * rejected.
 */
#define USF_VCTX_MAX 32
#define USF_FN_COUPLING_VCTX 65
int usf_coupling_additive_vctx_f32(const usf_coupling_desc* d, const float* ctx, int64_t ld_ctx, int32_t ctx_dim,
                                   const float* W_ctx_t, int64_t ldw_ctx, const float* b_ctx, usf_stream_t stream);
int usf_coupling_additive_vctx_variant(const usf_coupling_desc* d, int32_t ctx_dim);

/* usf_conv_ctx_wgrad_f32 (ABI 36; ks = 1, 3, 4 or 5 -- 5 on a 25-tap, 4 on a 16-tap instantiation of the same kernel, the latter in torch's placement, one zero before and two after): the weight gradient of the context channel of usf_conv2d_same_ctx_f32 (usflows_hip.h;
 * reference networks.py:513-680 under autograd),
 *   dw_ctx[co, t] = sum_b ctx[b * ctx_stride] * sum over the p whose tap t lands inside the image of dy[b, co, p]
 * dy [B, cout, H, W] contiguous fp32, dw_ctx [cout, ks * ks].  One block per output channel reads its dy plane once; the sums
 * run in a fixed order (same bits on every run) and need no workspace and no second launch.  The data channels' weight and
 * bias gradients are usf_conv_wgrad_f32's, the data gradient the usual transposed convolution over the cin data channels;
 * there is no gradient with respect to the context. */
int usf_conv_ctx_wgrad_f32(const float* dy, const float* ctx, int64_t ctx_stride, int64_t B, int64_t cout, int64_t H, int64_t W,
                           int64_t ks, float* dw_ctx, usf_stream_t stream);

/*
 * Gradients of the image-shaped coupling layer's pieces: what torch autograd computes for networks.py:40-122, 405-510 and the
 * 1 x 1 convolution of transforms.py:904-962 when Flow.fit (flows.py:113-210) trains an image flow.  All tensors contiguous
 * fp32; sums over the batch are deterministic (per-wave partial sums in the caller's workspace, added in a fixed order).
 *
 * usf_conv_wgrad_f32: weight and bias gradient of a stride-1 "same" convolution with kernel ks = 1 or 3,
 *     dW[co, ci, ky, kx] = sum_{b, p} dy[b, co, p] * xin[b, ci, p + (ky - ks/2, kx - ks/2)]     (nn.Conv2d weight layout [cout, cin, ks, ks])
 *     db[co]             = sum_{b, p} dy[b, co, p]                                             (db may be NULL)
 *   with xin = in_act(x - pre_sub[ci]) * in_mul -- the input transforms of usf_conv2d_same_f32 (in_act, in_mul) and of
 *   usf_channel_affine_f32 (pre_sub), each optional -- and zeros outside the image.  Exact fp32 products and sums on
 *   v_mfma_f32_16x16x4_f32.  Served: cin, cout multiples of 16 up to 64 (kernel 3: (cin / 16) * (cout / 16) <= 6 and neither of them 64), H * W <= 64, W >= 2, 16-byte
 *   aligned tensors; returns 1 (nothing written) for other shapes, 0 when done, < 0 on error.  workspace: at least
 *   usf_conv_wgrad_workspace(...) floats (0 = shape served neither with nor without in_mul; 64 -> 64 channels at kernel 1 and
 *   57 .. 64 pixels are served without in_mul only).  The DATA gradient of these layers is the forward entry point
 *   on the flipped, transposed weight (usf_conv2d_same_f32 / usf_pointwise_conv_f32 / usf_channel_affine_f32).
 * usf_layernorm_channels_bwd_f32: backward of usf_layernorm_channels_f32 (same x, gamma, eps, act, slope):
 *     dx [B, C, P]; dgamma_dbeta [2 C] = (sum dy * xhat, sum dy); workspace >= usf_layernorm_channels_bwd_workspace(B, C, P) floats.
 * usf_gated_residual_bwd_f32: backward of usf_gated_residual_f32 with respect to vg: dvg [B, 2C, P] =
 *     (dy * sigmoid(gate), dy * val * sigmoid(gate) * (1 - sigmoid(gate))); the gradient with respect to x is dy itself.
 */
/* Deferred sums of per-wave partial slots (the last stage of usf_conv_wgrad_f32) and many of them in ONE launch.
 * usf_conv_wgrad_deferred_f32 = usf_conv_wgrad_f32 that stops in front of that stage: job[0 .. 1] (HOST memory, two entries)
 * then describe what remains -- job[1] the final round that writes dW / db, job[0] the first round into the workspace's
 * scratch rows when there are more than 64 slots (job[0].nparts == 0: a single round).  dW / db stay UNWRITTEN until
 * usf_partial_sum_jobs_f32 launches containing first job[0] (if any), then job[1] have run in this stream order; the workspace
 * must stay alive until then.
 * usf_partial_sum_jobs_f32: jobs / block_job are DEVICE arrays: job j owns the blocks [first_block, first_block +
 * ceil(n / 64) * rows) -- ceil(n / 256) * rows when vec4 != 0 (mode 0, n a multiple of 4, 16-byte aligned part / out: four
 * columns per thread) -- and block_job[b] names block b's job (n_blocks entries).  Row r of a job sums the slots
 * [r * per, min((r + 1) * per, nparts)) in the order usf_conv_wgrad_f32's own rounds use: same bits.
 * Why: at the reference's training batch (32 rows, experiments/mnist/mnist.yaml:34) a backward pass of the live MNIST
 * configuration ends ~165 weight gradients with one or two such launches of a few microseconds each, all on the chain of
 * dependent launches that bounds the step; queued, they are two launches behind the pass. */
typedef struct usf_psum_job {
  const float* part; float* out; float* out2;
  int32_t nparts, n, mode, cin, cout, CIT, T, ntile;
  int32_t first_block, per, rows, vec4;
} usf_psum_job;
int usf_conv_wgrad_deferred_f32(const float* x, const float* dy, int64_t B, int64_t cin, int64_t cout, int64_t H, int64_t W, int64_t ks,
                                const float* in_mul, const float* pre_sub, int32_t in_act, float in_slope, float* dW, float* db,
                                float* workspace, int64_t workspace_floats, usf_psum_job* job, usf_stream_t stream);
int usf_partial_sum_jobs_f32(const usf_psum_job* jobs, const int32_t* block_job, int64_t n_blocks, usf_stream_t stream);
/* The weight-gradient kernel itself queued as well (small batches: one weight gradient occupies an eighth of the chip).
 * usf_conv_wgrad_plan_f32 = usf_conv_wgrad_deferred_f32 that launches NOTHING when the shape runs on the LDS-staged kernel: it
 * fills *wjob (HOST memory; blocks > 0) with that kernel's arguments -- the caller later runs all queued jobs of equal
 * (CIT, COT, T) with ONE usf_conv_wgrad_jobs_f32 launch (jobs / block_job DEVICE arrays as for usf_partial_sum_jobs_f32: job j
 * owns the blocks [first_block, first_block + blocks), first_block set by the caller; lds_bytes = the largest of the jobs')
 * and then the sums job[0 .. 1] describe.  x, dy, in_mul, pre_sub and the workspace must stay alive and unchanged until then.
 * wjob->blocks == 0 on return: the shape runs on the direct kernel-1 form, which HAS been launched (only the sums remain). */
typedef struct usf_wgrad_job {
  unsigned char args[192];                      /* the kernel's arguments (opaque) */
  int32_t CIT, COT, T, blocks, lds_bytes, first_block;
} usf_wgrad_job;
int usf_conv_wgrad_plan_f32(const float* x, const float* dy, int64_t B, int64_t cin, int64_t cout, int64_t H, int64_t W, int64_t ks,
                            const float* in_mul, const float* pre_sub, int32_t in_act, float in_slope, float* dW, float* db,
                            float* workspace, int64_t workspace_floats, usf_psum_job* job, usf_wgrad_job* wjob, usf_stream_t stream);
int usf_conv_wgrad_jobs_f32(const usf_wgrad_job* jobs, const int32_t* block_job, int64_t n_blocks, int32_t CIT, int32_t COT, int32_t T,
                            int32_t lds_bytes, usf_stream_t stream);
int64_t usf_conv_wgrad_workspace(int64_t B, int64_t cin, int64_t cout, int64_t H, int64_t W, int64_t ks);
int usf_conv_wgrad_f32(const float* x, const float* dy, int64_t B, int64_t cin, int64_t cout, int64_t H, int64_t W, int64_t ks,
                       const float* in_mul, const float* pre_sub, int32_t in_act, float in_slope, float* dW, float* db,
                       float* workspace, int64_t workspace_floats, usf_stream_t stream);
int64_t usf_layernorm_channels_bwd_workspace(int64_t B, int64_t C, int64_t P);
int usf_layernorm_channels_bwd_f32(const float* x, const float* dy, float* dx, int64_t B, int64_t C, int64_t P, const float* gamma,
                                   float eps, int32_t act, float slope, float* dgamma_dbeta, float* workspace,
                                   int64_t workspace_floats, usf_stream_t stream);
int usf_gated_residual_bwd_f32(const float* dy, const float* vg, float* dvg, int64_t B, int64_t CP, usf_stream_t stream);

/*
 * usf_conv_wgrad_variant (internal version 6): which kernel a call of usf_conv_wgrad_f32 (or its deferred / plan forms)
 * launches and how -- answered by the planning function the entry points themselves launch from (host only, nothing is
 * launched, no tensor pointer exists).
 * Query: B, cin, cout, H, W, ks, masked (1: the call passes in_mul); cus and blocks_per_cu: the device's compute units and the
 * occupancy answer for the kernel instance (resident blocks per compute unit) -- 0 asks the device, as a launch does; > 0
 * plans for the stated value (works without a GPU).  The tuning knobs in force are honoured as a launch honours them:
 * conv_wgrad_rsplit (0: one wave per sample) and conv_wgrad_blocks (> 0: caps the grid; default 0 = the occupancy cap alone --
 * a test aid: with it a batch of a few dozen samples gives every wave several samples).
 * Answer: kernel 0 not served (the call returns 1), 1 the LDS-staged kernel conv_wgrad_kernel<CIT, COT, T>, 2 the direct 1 x 1
 * kernel conv_wgrad_k1_kernel<CIT, COT>; rsplit waves per sample, grid blocks, lds_bytes; the staging geometry (row stride S,
 * first pixel at base, first position read q0, channel stride CS, nch position chunks, nacc floats per partial slot,
 * tab_floats of tables in front of the waves' images); the sum over the slots = 4 * blocks partial slots in `rounds` (1 or
 * 2) rounds, the first of two with rows_used rows of `per` slots; max_samples_per_wave = ceil(B / (slots / rsplit));
 * blocks_per_cu / cus: the values the plan was made with.  Returns 0 or -1 (null pointer).
 * usf_layernorm_channels_bwd_variant: the same for usf_layernorm_channels_bwd_f32: kernel 1 = one thread per pixel
 * (layernorm_channels_bwd_kernel<width, false>, width = CMAX 16 / 32 / 64), 2 = two lanes per pixel
 * (layernorm_channels_bwd2_kernel<width>, width = CPT = C / 2 for C = 16, 32, 48, 64); 0: the sizes are refused.
 */
typedef struct usf_conv_wgrad_query {
  int64_t B, cin, cout, H, W, ks;
  int32_t masked, cus, blocks_per_cu, reserved;
} usf_conv_wgrad_query;
typedef struct usf_conv_wgrad_info {
  int32_t kernel, CIT, COT, T, rsplit, blocks, lds_bytes;
  int32_t S, base, q0, CS, nch, nacc, tab_floats;
  int32_t slots, rounds, per, rows_used, max_samples_per_wave;
  int32_t blocks_per_cu, cus, reserved;
} usf_conv_wgrad_info;
int usf_conv_wgrad_variant(const usf_conv_wgrad_query* q, usf_conv_wgrad_info* out);
typedef struct usf_ln_bwd_info {
  int32_t kernel, width, blocks, slots, rounds, per, rows_used, reserved;
} usf_ln_bwd_info;
int usf_layernorm_channels_bwd_variant(int64_t B, int64_t C, int64_t P, usf_ln_bwd_info* out);

/*
 * usf_conv_wgrad_wide_f32 (an addition: USF_INTERNAL_VERSION is unchanged): the contract and the argument list of usf_conv_wgrad_f32 -- dW, db of a stride-1
 * "same" convolution with kernel 1 or 3 from x (with the input transforms in_act, in_mul, pre_sub) and dy, exact fp32 on
 * v_mfma_f32_16x16x4_f32, deterministic -- for the shapes that entry point refuses: one 256-thread block stages one sample at a
 * time into LDS and the (cout tile, cin tile, tap) accumulator tiles are dealt over its four waves (usf_conv_wgrad_wide.hip).
 * Served: 1 <= cin, cout <= 64 (ANY value: channel tiles are zero-padded to 16 in LDS), 1 <= H * W <= 256 (W == 1 included),
 * B >= 1, tensors 4-byte aligned, provided the sample's LDS image fits 160 KiB:
 *     kernel 3: S = W + 1, n = 4 * ceil(((H - 1) * S + W) / 4), CSy = 2odd(n), CSx = 2odd(n + 2 * S + 2)
 *     kernel 1: CSx = CSy = 2odd(4 * ceil(H * W / 4))             (2odd(v): the smallest 2 * odd number >= v)
 *     4 * ((16 * ceil(cin / 16) + 1) * CSx + 16 * ceil(cout / 16) * CSy) <= 163840 bytes     (+ 1: a row of ones, db's operand)
 * -- 64 + 64 channels at 16 x 16 take 150 744 bytes; tall maps of very few columns and many channels do not
 * (the pad column weighs most there: usf_conv_wgrad_wide_variant answers for a shape).  Returns 1 (nothing written) for other shapes, 0 when done, < 0 on error (nothing
 * written either).  workspace: at least usf_conv_wgrad_wide_workspace(...) floats (0: shape not served); it depends on the
 * device's compute units.  Small maps (H * W <= 64) are served too: the same sums as usf_conv_wgrad_f32 in another order.
 * Two or three launches in stream order (the kernel, one or two rounds of the sum), no host synchronisation.
 *
 * usf_conv_wgrad_wide_variant: the plan such a call launches from, asked instead of launched (host only; q->masked is
 * ignored: both forms run the same kernel; cus > 0 plans for that many compute units and blocks_per_cu > 0 for that
 * residency -- with cus stated it needs no GPU).  served 0 / 1; tiles = COT * (CIT * T + 1) accumulator tiles (+ 1: db), dealt over
 * wave_groups (2 or 4) groups of waves with tiles_per_wave each -- the kernel's instantiation, one of
 * usf_conv_wgrad_wide_instances -- while position_parts = 4 / wave_groups waves share a tile and split the nch position chunks;
 * blocks (the grid: min(B, cus * min(blocks_per_cu, 2))), lds_bytes, the staging geometry (S, q0, CSx, CSy, nch), nacc floats
 * per partial slot, slots = blocks * position_parts summed in `rounds` (1 or 2) rounds, the first of two with rows_used rows
 * of `per` slots; max_samples_per_block = ceil(B / blocks).
 * usf_conv_wgrad_wide_instances: writes the tiles_per_wave values the kernel is instantiated for (up to cap) and returns
 * their count.
 */
typedef struct usf_conv_wgrad_wide_info {
  int32_t served, CIT, COT, T, tiles, tiles_per_wave, wave_groups, position_parts;
  int32_t blocks, lds_bytes, S, q0, CSx, CSy, nch, nacc;
  int32_t slots, rounds, per, rows_used, max_samples_per_block, blocks_per_cu, cus, reserved;
} usf_conv_wgrad_wide_info;
int64_t usf_conv_wgrad_wide_workspace(int64_t B, int64_t cin, int64_t cout, int64_t H, int64_t W, int64_t ks);
int usf_conv_wgrad_wide_f32(const float* x, const float* dy, int64_t B, int64_t cin, int64_t cout, int64_t H, int64_t W, int64_t ks,
                            const float* in_mul, const float* pre_sub, int32_t in_act, float in_slope, float* dW, float* db,
                            float* workspace, int64_t workspace_floats, usf_stream_t stream);
int usf_conv_wgrad_wide_variant(const usf_conv_wgrad_query* q, usf_conv_wgrad_wide_info* out);
int usf_conv_wgrad_wide_instances(int32_t* out, int32_t cap);

/*
 * usf_conv_wgrad_k5_f32 (an addition: USF_INTERNAL_VERSION is unchanged): the contract and the argument list of
 * usf_conv_wgrad_wide_f32 for kernel 5 -- dW [cout, cin, 5, 5] and db [cout] (or NULL) from x (with in_act, in_mul, pre_sub) and
 * dy, exact fp32 on v_mfma_f32_16x16x4_f32, fixed-order sums, the same bits on every run, no atomics (usf_conv_wgrad_k5.hip).
 * The wide kernel's design -- a 256-thread block owns one sample at a time in LDS -- with the 25 taps dealt over the grid:
 * blockIdx.y is a tap row of 5, so a wave holds at most 21 accumulator tiles; the bias tiles belong to tap row 0 alone; every
 * (tap row, block) owns its partial slot.  Served: ks == 5 only (usf_conv_wgrad_f32 and usf_conv_wgrad_wide_f32 keep refusing
 * it), 1 <= cin, cout <= 64 (any value), 1 <= H * W <= 256 at every pixel count (no 64-pixel split), B >= 1, provided
 *     S = W + 2, n = 4 * ceil(((H - 1) * S + W) / 4), CSy = 2odd(n), CSx = 2odd(n + 4 * S + 5)
 *     4 * ((16 * ceil(cin / 16) + 1) * CSx + 16 * ceil(cout / 16) * CSy) <= 163840 bytes
 * (64 + 64 channels up to 15 x 15; 16 x 16 up to 48 + 64).  Returns 1 (nothing written) for other shapes, 0 when done, < 0 on
 * error.  workspace: at least usf_conv_wgrad_k5_workspace(...) floats (0: not served; it depends on the device's compute units).
 * Two or three launches in stream order, no host synchronisation.
 * usf_conv_wgrad_k5_variant answers with the plan in a usf_conv_wgrad_wide_info (host only; cus > 0: no GPU needed): T = 5 taps
 * per tap row, position_parts = 5 tap rows (grid.y), wave_groups = 4, tiles = COT * (CIT * 5 + 1) accumulator tiles of tap row
 * 0, tiles_per_wave = ceil(tiles / 4) rounded up to one of usf_conv_wgrad_k5_instances, blocks = grid.x = min(B, ceil(cus *
 * min(blocks_per_cu, 2) / 5)), slots = blocks partial slots per tap row of nacc floats, summed per tap row in `rounds` rounds.
 */
int64_t usf_conv_wgrad_k5_workspace(int64_t B, int64_t cin, int64_t cout, int64_t H, int64_t W, int64_t ks);
int usf_conv_wgrad_k5_f32(const float* x, const float* dy, int64_t B, int64_t cin, int64_t cout, int64_t H, int64_t W, int64_t ks,
                          const float* in_mul, const float* pre_sub, int32_t in_act, float in_slope, float* dW, float* db,
                          float* workspace, int64_t workspace_floats, usf_stream_t stream);
int usf_conv_wgrad_k5_variant(const usf_conv_wgrad_query* q, usf_conv_wgrad_wide_info* out);
int usf_conv_wgrad_k5_instances(int32_t* out, int32_t cap);

/*
 * usf_conv_wgrad_k4_f32 (an addition: USF_INTERNAL_VERSION is unchanged): the same for kernel 4 in torch's "same" placement,
 *     dW[co, ci, ty, tx] = sum_{b, p} dy[b, co, p] * xin[b, ci, p + (ty - 1, tx - 1)],   db[co] = sum_{b, p} dy[b, co, p]
 * -- an instantiation of usf_conv_wgrad_k5_f32's kernel with FOUR tap rows of FOUR taps dealt over grid.y (64 -> 64 channels:
 * 4 * (4 * 4 + 1) = 68 tiles in tap row 0, 17 per wave), the same LDS geometry and size rule, the same instantiation set.
 * Served: ks == 4 only (usf_conv_wgrad_k5_f32 keeps refusing it).  In the variant's answer T = 4 and position_parts = 4.
 */
int64_t usf_conv_wgrad_k4_workspace(int64_t B, int64_t cin, int64_t cout, int64_t H, int64_t W, int64_t ks);
int usf_conv_wgrad_k4_f32(const float* x, const float* dy, int64_t B, int64_t cin, int64_t cout, int64_t H, int64_t W, int64_t ks,
                          const float* in_mul, const float* pre_sub, int32_t in_act, float in_slope, float* dW, float* db,
                          float* workspace, int64_t workspace_floats, usf_stream_t stream);
int usf_conv_wgrad_k4_variant(const usf_conv_wgrad_query* q, usf_conv_wgrad_wide_info* out);
int usf_conv_wgrad_k4_instances(int32_t* out, int32_t cap);

/*
 * usf_conv_wgrad_band_f32 (an addition: USF_INTERNAL_VERSION is unchanged): the contract and the argument list of
 * usf_conv_wgrad_wide_f32 -- dW [cout, cin, ks, ks] and db [cout] (or NULL) of a stride-1 "same" convolution with kernel 1 or 3
 * from x (with in_act, in_mul, pre_sub) and dy, exact fp32 on v_mfma_f32_16x16x4_f32, fixed-order sums, the same bits on every
 * run, no atomics -- for the feature maps that kernel refuses: 257 .. 4096 pixels (usf_conv_wgrad_band.hip).  The wide kernel's
 * decomposition with another GROUP: a persistent 256-thread block stages a band of RB consecutive rows of ONE sample (x rows
 * r0 - pad .. r0 + RB - 1 + pad, dy rows r0 .. r0 + RB - 1; group g = sample g / bands, band g % bands), walks its groups in
 * ascending order and keeps its accumulators across them.  One more argument, band_rows: 0 = the plan's band, > 0 caps it (a test
 * and measurement aid, as usf_conv2d_same_band_f32 has).
 * Served: ks 1 or 3, 1 <= cin, cout <= 64 (any value), 1 <= W <= 64 (W == 1 included), H * W <= 4096 (small maps too: the wide
 * kernel's sums in another order), B >= 1, B * bands < 2^31, provided a band fits the 160 KiB of LDS:
 *     kernel 3: S = W + 1, n = 4 * ceil(((RB - 1) * S + W) / 4), CSy = 2odd(n), CSx = 2odd(n + 2 * S + 2)
 *     kernel 1: CSx = CSy = 2odd(4 * ceil(RB * W / 4))
 *     4 * ((16 * ceil(cin / 16) + 1) * CSx + 64 + 16 * ceil(cout / 16) * CSy) <= 163840 bytes
 * (+ 1 row and 64 floats: db's operand, ones in every 16th chunk of four positions, read by column j of the bias tile 16 - j
 * chunks in, so that db is the fixed-order sum of 16 chains a sixteenth as long -- a block's chains span all its groups)
 * -- and, at kernel 3, that the largest such RB is at least 4 or the whole map (refused: 49 .. 64 channels on both sides at
 * W = 64, where one to three rows fit and the halo rows would outweigh the band).  The plan (usf_conv_wgrad_band_plan.h) takes the
 * largest RB that fits; a batch with fewer groups than compute units takes a lower band, down to 4 rows; the bands are evened
 * out (the same number of bands, ceil(H / bands) rows each); band_rows caps the result as it is.  Returns 1 (nothing written) for
 * other shapes, 0 when done, < 0 on error (nothing written either).  workspace: at least usf_conv_wgrad_band_workspace(...,
 * band_rows) floats (0: not served); it depends on the device's compute units and on the tuning knob conv_wgrad_band_blocks
 * (> 0 caps the grid: a test aid, as conv_wgrad_blocks).  Two or three launches in stream order, no host synchronisation.
 *
 * usf_conv_wgrad_band_variant: the whole plan such a call launches from (host only; cus > 0 plans for that many compute units and
 * needs no GPU, blocks_per_cu > 0 for that residency).  served 0 / 1; band_rows (of this launch), best_rows (the plan's own
 * choice, before the cap), fit_rows (the most the LDS holds), bands, last_rows (of a sample's last band), staged_rows = band_rows
 * + 2 * pad, groups = B * bands, grid = min(groups, cus * min(blocks_per_cu, 2)) under the knob, lds_bytes; tiles, tiles_per_wave
 * (the instantiation, one of usf_conv_wgrad_band_instances), wave_groups, position_parts, slots = grid * position_parts summed
 * in `rounds` (1 or 2) rounds, the first of two with rows_used rows of `per` slots, as in usf_conv_wgrad_wide_info;
 * max_groups_per_block = ceil(groups / grid); the geometry (S, q0, CSx, CSy, nch, nacc); and the multiply-high divisions of the
 * staging loops: m_x, m_y, m_w = ceil(2^32 / d) for d = staged_rows * W, band_rows * W, W (0: d == 1), applied to dividends up to
 * max_dividend (m_w: below staged_rows * W).  usf_sizeof_desc reports sizeof(usf_conv_wgrad_band_query|_info) for kind 29|30.
 */
typedef struct usf_conv_wgrad_band_query {
  int64_t B, cin, cout, H, W, ks;
  int32_t band_rows, cus, blocks_per_cu, reserved;
} usf_conv_wgrad_band_query;
typedef struct usf_conv_wgrad_band_info {
  int32_t served, band_rows, best_rows, fit_rows, bands, last_rows, staged_rows, groups;
  int32_t grid, lds_bytes, CIT, COT, T, tiles, tiles_per_wave, wave_groups;
  int32_t position_parts, slots, rounds, per, rows_used, max_groups_per_block, blocks_per_cu, cus;
  int32_t S, q0, CSx, CSy, nch, nacc, max_dividend, reserved;
  uint32_t m_x, m_y, m_w, reserved2;
} usf_conv_wgrad_band_info;
int64_t usf_conv_wgrad_band_workspace(int64_t B, int64_t cin, int64_t cout, int64_t H, int64_t W, int64_t ks, int64_t band_rows);
int usf_conv_wgrad_band_f32(const float* x, const float* dy, int64_t B, int64_t cin, int64_t cout, int64_t H, int64_t W, int64_t ks,
                            const float* in_mul, const float* pre_sub, int32_t in_act, float in_slope, float* dW, float* db,
                            float* workspace, int64_t workspace_floats, int64_t band_rows, usf_stream_t stream);
int usf_conv_wgrad_band_variant(const usf_conv_wgrad_band_query* q, usf_conv_wgrad_band_info* out);
int usf_conv_wgrad_band_instances(int32_t* out, int32_t cap);

/*
 * usf_conv2d_same_pad_f32 (an addition: USF_INTERNAL_VERSION is unchanged): usf_conv2d_same_f32 (usflows_hip.h) with the
 * placement of the zero padding stated -- pad_before zeros before the image and ks - 1 - pad_before after it, in each axis:
 *     y[p] = sum_t w[t] x[p + t - pad_before].
 * pad_before == (ks - 1) / 2 is usf_conv2d_same_f32 itself (same kernels, same bits).  At an even ks (4) pad_before == ks / 2 is
 * the MIRRORED placement, what the data gradient of a "same" convolution with an even kernel is on the flipped, transposed
 * weight (usf_conv2d_weight_planes_f32 with transposed = 1): dx[q] = sum_s w[3 - s] dy[q + s - 2].  Every other pad_before, and
 * gate_x != NULL with the mirrored placement, is refused with -2 and nothing is launched.  Only the training path's data
 * gradient calls it (captured as a graph, never recorded as an op list).
 * usf_conv2d_same_pad_fits: usf_conv2d_same_fits for a placement (0 for a pad_before the call refuses).  Both placements have
 * the same padded image, (H + ks - 1) x (W + ks - 1), hence the same plan and LDS footprint: the answer for the mirrored
 * placement IS usf_conv2d_same_fits' and usf_conv2d_same_variant's.
 */
int usf_conv2d_same_pad_fits(int64_t cin, int64_t cout, int64_t H, int64_t W, int64_t ks, int64_t pad_before);
int usf_conv2d_same_pad_f32(const float* x, float* y, int64_t B, int64_t cin, int64_t cout, int64_t H, int64_t W, int64_t ks,
                            int64_t pad_before, const void* w_planes, const float* bias, const float* in_mul, int32_t in_act,
                            float in_slope, int32_t out_act, float out_slope, const float* gate_x, int64_t gate_channels,
                            usf_stream_t stream);

/* usf_conv2d_weight_planes_f32(transposed = 2) for MANY weights in one launch.  jobs / block_job are DEVICE arrays (as for
 * usf_partial_sum_jobs_f32): job j splits the fp32 weight w [cout, cin, ks, ks] (any ks the single call takes; ks = 4: the second
 * set is for the mirrored placement, usf_conv2d_same_pad_f32) into its planes followed by the planes of its
 * data-gradient convolution, at planes_base + out_off (bf16 elements; usf_conv2d_weight_elems(cin, cout, ks) +
 * usf_conv2d_weight_elems(cout, cin, ks) of them), and owns the blocks [first_block, first_block + ceil(max of the two
 * [rows x K] sizes / 256)); block_job[b] names block b's job.  Same bits as the single launches. */
typedef struct usf_wplanes_job {
  const float* w; int64_t out_off;
  int32_t cin, cout, ks, first_block;
} usf_wplanes_job;
int usf_conv2d_weight_planes_batch_f32(const usf_wplanes_job* jobs, const int32_t* block_job, int64_t n_blocks, void* planes_base,
                                       usf_stream_t stream);

/* usf_gated_tail_bwd_f32: the backward of usf_gated_tail_f32 (usflows_hip.h, same operands) in ONE launch.  It replaces the
 * chain usf_layernorm_channels_bwd_f32 -> usf_gated_residual_bwd_f32 -> usf_pointwise_conv_f32 on a transposed copy of W ->
 * usf_conv_wgrad_f32 (kernel 1): the backward recomputes val / gate / r from (h, x) and writes dx [B, C, P] (the skip branch), dh [B, C, P] and
 * dparams = [dW (2 C C) | dbias (2 C) | dgamma (C) | dbeta (C)] (the last two only with a layer norm); dvg [B, 2 C, P] =
 * d[val, gate] is written when the pointer is not NULL.  workspace >= usf_gated_tail_workspace floats.
 * job == NULL: dparams is complete when the call's launches have run; else job[0 .. 1] (HOST memory) describe its last
 * sum for usf_partial_sum_jobs_f32 as usf_conv_wgrad_deferred_f32 does (nparts == 0: nothing to do).
 * Eight lanes share a pixel: made for few pixels (a 32-row training batch); HBM traffic 4 C (3 + 2) bytes per pixel backward. */
int64_t usf_gated_tail_workspace(int64_t B, int64_t C, int64_t P);
int usf_gated_tail_bwd_f32(const float* h, const float* x, const float* dy, float* dx, float* dh, float* dvg, int64_t B, int64_t C,
                           int64_t P, const float* W, const float* bias, int32_t in_act, float in_slope, int32_t post_act,
                           float post_slope, const float* ln_gamma, const float* ln_beta, float ln_eps, float* dparams,
                           float* workspace, int64_t workspace_floats, struct usf_psum_job* job, usf_stream_t stream);

/*
 * usf_channel_affine_bwd_f32 (an addition: USF_INTERNAL_VERSION is unchanged): the WHOLE backward of usf_channel_affine_f32
 * (usflows_hip.h) with few channels in ONE launch plus the sum over its per-block slots -- contiguous fp32 [B, C, P] tensors:
 *     dx[b, c', p] = sum_c W[c, c'] * dy[b, c, p]                       (W [C, C] as the forward used it; dx may be NULL)
 *     dW[c, c']    = sum_{b, p} dy[b, c, p] * (x[b, c', p] - pre_sub[c'])    (pre_sub [C] or NULL)
 *     db[c]        = sum_{b, p} dy[b, c, p]                             (db may be NULL; else db == dW + C * C: the last sum
 *                                                                        writes dW and db as one buffer of C * C + C floats)
 * Served: 1 <= C <= 12, any P >= 1, any B >= 1; other sizes return 1 and write nothing; B == 0 returns 0 and writes nothing;
 * < 0 on error (nothing written either).  A thread owns whole pixels and keeps the C^2 + C sums in registers (channels padded
 * to 4, 8 or 12; channels >= C are never loaded or stored); 16-byte loads and stores where P % 4 == 0 and x, dy, dx are 16-byte
 * aligned, one float at a time otherwise.  Exact fp32: fmaf chains in ascending channel order, every thread's pixels in
 * ascending order, a fixed shuffle order inside a wave, the four waves in ascending order through LDS, one slot per block,
 * the slots by the sum usf_gated_tail_bwd_f32 uses (job == NULL: at once; else job[0 .. 1], HOST memory, describe it for
 * usf_partial_sum_jobs_f32 as usf_conv_wgrad_deferred_f32 does).  The grid depends on the sizes and the form alone -- at most
 * 256 blocks; the tuning aid channel_affine_bwd_blocks > 0 lowers that cap (tests: several loop trips at a small size) --
 * so two runs give the same bits.  No matrix instructions, no atomics.
 * workspace: at least usf_channel_affine_bwd_workspace(B, C, P) floats (0: sizes not served; host only).
 * usf_channel_affine_bwd_variant (host only, launches nothing): the plan such a call launches from.  Query: the sizes,
 * aligned16 (1: x, dy and dx are 16-byte aligned), want_bias (1: db is asked for), grid_cap (> 0: plan for this cap on the grid
 * instead of the tuning aid's / the default -- works without a GPU, as everything here does).  Answer: served 0 / 1, width
 * (4 / 8 / 12: the instantiation's padded channel count), vec (1: the 16-byte form), blocks, trips (loop trips of the busiest
 * thread), slot_floats (C * C [+ C]), slots (= blocks) summed in `rounds` (1 or 2) rounds, the first of two with rows_used rows
 * of `per` slots; grid_cap: the cap the plan was made with.  Returns 0 or -1 (null pointer).
 * usf_sizeof_desc reports sizeof(usf_channel_affine_bwd_query|usf_channel_affine_bwd_info) for kind 25|26.
 */
typedef struct usf_channel_affine_bwd_query {
  int64_t B, C, P;
  int32_t aligned16, want_bias, grid_cap, reserved;
} usf_channel_affine_bwd_query;
typedef struct usf_channel_affine_bwd_info {
  int32_t served, width, vec, blocks, trips, slot_floats;
  int32_t slots, rounds, per, rows_used, grid_cap, reserved;
} usf_channel_affine_bwd_info;
int64_t usf_channel_affine_bwd_workspace(int64_t B, int64_t C, int64_t P);
int usf_channel_affine_bwd_f32(const float* x, const float* dy, float* dx, int64_t B, int64_t C, int64_t P, const float* W,
                               const float* pre_sub, float* dW, float* db, float* workspace, int64_t workspace_floats,
                               struct usf_psum_job* job, usf_stream_t stream);
int usf_channel_affine_bwd_variant(const usf_channel_affine_bwd_query* q, usf_channel_affine_bwd_info* out);

/* A data-gradient convolution with the factors of the layer's INPUT transforms in its output stream:
 *   y = conv(x) * (gate_h > 0 ? 1 : gate_slope) * gate_mul          (gate_add == NULL)
 *   y = gate_add + conv(x) * (gate_h > 0 ? 1 : gate_slope)          (gate_add != NULL; then gate_mul must be NULL)
 * gate_h [B, cout, H, W] = the forward layer's input (its (Leaky)ReLU's derivative; gate_slope 0 = ReLU, 1 = no nonlinearity),
 * gate_mul [cout * H * W] or NULL = the forward layer's input mask, gate_add [B, cout, H, W] or NULL = the gradient that
 * reaches the same tensor along another branch (the forward input forks: GatedConv's skip connection, networks.py:108-122).
 * The arithmetic of usf_conv2d_same_f32 followed by usf_act_grad_f32 and the mask product / the sum, in one pass.  Returns 0
 * when done, 1 when the shape is not served by this form, < 0 on error.  Served: what usf_conv2d_same_res_f32 serves (3 x 3,
 * 16 / 32 / 48 -> 16 / 32 / 48 / 64 channels, H W <= 64, every tensor 16-byte aligned); under the tuning knob conv_wsp=0 (the
 * register-weight kernel) no 48 channels and no gate_add form.  usf_conv2d_same_variant answers for a given call. */
int usf_conv2d_same_gate_f32(const float* x, float* y, int64_t B, int64_t cin, int64_t cout, int64_t H, int64_t W, int64_t ks,
                             const void* w_planes, const float* gate_h, float gate_slope, const float* gate_mul,
                             const float* gate_add, usf_stream_t stream);

/*
 * usf_conv2d_same_variant (internal version 5): which kernel a call of the "same" convolution's entry points launches, and
 * how -- answered by the planning functions the entry points themselves launch from (host only, nothing is launched, no
 * tensor pointer exists).  Four kernels serve the five entry points:
 *   1  conv2d_same_bf16x3_kernel<CTX>            every shape usf_conv2d_same_f32 accepts, gated mode, 4-byte tensor accesses
 *   2  conv2d_same_wreg_kernel<NB, CP, NCT, CTX> 3 x 3, 16 / 32 -> 16 / 32 / 64 channels, H W <= 64; only under the tuning
 *                                                knob conv_wsp=0; no gate-add form, residual forms up to 8192 outputs per group
 *   3  conv2d_same_wsp_kernel<NB, CP, NCT, CTX>  3 x 3, 16 / 32 / 48 -> 16 / 32 / 48 / 64 channels, H W <= 64
 *   4  conv2d_same_stream_kernel<NR, CTX, KSZ>   5 x 5 and 4 x 4 (KSZ; an addition: USF_INTERNAL_VERSION is unchanged, the struct is as it
 *                                                was), plain / ctx calls where kernel 1 cannot hold the 25 taps' weight planes
 *                                                and two padded samples in the LDS: the group's image stays resident, the weights
 *                                                move through a ring of two K slabs, one barrier per slab (usf_conv_stream.hip).
 *                                                ks = 4 / 5 runs on kernel 1 where its best S is >= 2 (or nothing else fits), else here
 * Kernels 2 and 3 want (cin H W) and (cout H W) multiples of 4 and every tensor 16-byte aligned; a plain / ctx call they do
 * not serve runs on kernel 1, a res / gate call they do not serve is answered with return code 1 (kernel 0 here).
 * Query: entry (USF_CONV_ENTRY_*; GATED: usf_conv2d_same_f32 with gate_x, cout = the packed row count), B, cin, cout, H, W,
 * ks (1, 3, 4 or 5; the answer at ks = 4 holds for both placements of its zeros: the plans do not look at the placement),
 * aligned (1: every tensor pointer is 16-byte aligned), cus (0: ask the device; > 0: plan for that many compute units --
 * works without a GPU).  The tuning knobs in force (conv_wreg, conv_wsp, conv_small_s) are honoured as a launch honours them.
 * Answer: kernel (0: not served / refused); S samples per group, groups = ceil(B / S), grid blocks, lds_bytes; for kernels 2
 * and 3 the instantiation (NB k-blocks, CP padded input channels, NCT output tiles) and the largest n each magic-number
 * division umulhi(n, m) is applied to (max_mHW / mW / mSE / mSO; -1: that division is not made); for kernel 1 the patch shape
 * (PC, PR) in 16-row tiles of a full group and of the last group (they differ when the last group is ragged); for kernel 4
 * NB = 32-value k-blocks per slab (2: a slab of 64 K values, a tap at 64 padded channels; 1: half of that, where only it brings a
 * second sample into the LDS), CP = padded input channels, NCT = slabs in the ring (2), PC = 2 and PR = NR, the 16-row tiles
 * per wave of the instantiation (1, 2, 4); CTX: the context instantiation.  Returns 0, -1 (null pointer) or -2 (bad entry).
 */
#define USF_CONV_ENTRY_PLAIN 0
#define USF_CONV_ENTRY_CTX 1
#define USF_CONV_ENTRY_RES 2
#define USF_CONV_ENTRY_GATE_MUL 3
#define USF_CONV_ENTRY_GATE_ADD 4
#define USF_CONV_ENTRY_GATED 5
typedef struct usf_conv_variant_query {
  int32_t entry, aligned;
  int64_t B, cin, cout, H, W, ks;
  int32_t cus, reserved;
} usf_conv_variant_query;
typedef struct usf_conv_variant {
  int32_t kernel, S;
  int64_t grid, groups, lds_bytes;
  int32_t NB, CP, NCT, CTX;
  int32_t PC_full, PR_full, PC_last, PR_last;
  int32_t max_mHW, max_mW, max_mSE, max_mSO;
} usf_conv_variant;
int usf_conv2d_same_variant(const usf_conv_variant_query* q, usf_conv_variant* out);

/*
 * usf_conv2d_same_band_f32 (an addition: USF_INTERNAL_VERSION is unchanged): the "same" convolution of usf_conv2d_same_f32 /
 * usf_conv2d_same_ctx_f32 (usflows_hip.h; ctx == NULL: the plain form, else ctx / ctx_stride / w_ctx as there) for feature maps
 * of up to 4096 pixels, on a fifth kernel, conv2d_same_band_kernel<CTX> (usf_conv_band.hip): a group of a persistent block is a
 * band of consecutive output rows of ONE sample, its LDS image (rows + ks - 1) x (W + ks - 1) positions beside the resident
 * weight planes.  Same arithmetic (bf16x3, six matrix instructions per product, k-blocks in order) and the same weight planes,
 * exactly as usf_conv2d_weight_planes_f32 makes them; an output element's bits depend on neither the band height nor the batch.
 * Served: ks 1 or 3, stride 1, zero "same" padding, 1 <= cin, cout <= 64, W <= 64, H W <= 4096 (maps of 256 pixels and fewer
 * included), B >= 1, the weight planes and a band within 158 KiB of LDS and 16 register-staged iterations per thread, and at
 * ks = 3 a best band of at least 4 output rows (or the whole map).  No gated mode, no fused residual, no gate forms, inference
 * only; no USF_FN_* id (a pass that calls it is not recorded as an op list).
 * band_rows: 0 = the plan's band; > 0 caps the band at that many output rows (a measurement and test aid).
 * Returns 0, 1 for a valid shape that is not served (nothing is launched), < 0 on bad arguments (usf_last_error()).
 * usf_conv2d_same_band_fits (host only): output rows per band the plan would use, 0 = not served.
 * usf_conv2d_same_band_variant (host only, nothing is launched): the plan of such a call.  Query: the sizes, ctx (1: the context
 * form), band_rows as above, cus (0: ask the device; > 0: plan for that many compute units -- works without a GPU).  Answer:
 * served 0 / 1; band_rows, bands per sample, last_rows (output rows of a sample's last band), groups = B * bands, grid blocks,
 * lds_bytes, stage_iters (register-staged iterations per thread, at most 16), CTX, the patch shape (PC, PR) in 16-row tiles of a
 * full band and of a last band; best_rows (the shape's band before the cap) and weight_bytes (LDS bytes of the weight planes)
 * are filled for refused shapes too where the sizes are in range.  Returns 0 or -1 (null pointer).
 * usf_sizeof_desc reports sizeof(usf_conv_band_query|usf_conv_band_info) for kind 27|28.
 */
typedef struct usf_conv_band_query {
  int64_t B, cin, cout, H, W, ks;
  int32_t ctx, band_rows, cus, reserved;
} usf_conv_band_query;
typedef struct usf_conv_band_info {
  int32_t served, band_rows, bands, last_rows;
  int64_t groups, grid, lds_bytes, weight_bytes;
  int32_t stage_iters, CTX, PC_full, PR_full, PC_last, PR_last, best_rows, reserved;
} usf_conv_band_info;
int usf_conv2d_same_band_fits(int64_t cin, int64_t cout, int64_t H, int64_t W, int64_t ks);
int usf_conv2d_same_band_f32(const float* x, float* y, int64_t B, int64_t cin, int64_t cout, int64_t H, int64_t W, int64_t ks,
                             const void* w_planes, const float* bias, const float* in_mul, int32_t in_act, float in_slope,
                             int32_t out_act, float out_slope, const float* ctx, int64_t ctx_stride, const float* w_ctx,
                             int64_t band_rows, usf_stream_t stream);
int usf_conv2d_same_band_variant(const usf_conv_band_query* q, usf_conv_band_info* out);

/* which instantiation of usf_gemm_planes_bf16x3 serves the descriptor (nothing is launched): 5000 + 10 TN + (1: fp32 output, 0: planes output),
 * TN = column-block width in 32-feature blocks (4 or 5, whichever pads the output less); 0 for empty extents */
int usf_gemm_planes_variant(const usf_gemm_planes_desc* d);

/* which instantiation of coupling_planes_kernel serves the descriptor as usf_coupling_planes (has_ctx == has_side == 0),
 * usf_coupling_planes_ctx (has_ctx != 0) or usf_coupling_planes_side (has_side != 0) -- an ADDED entry point, as the pair above.
 * Nothing is launched and no pointer is dereferenced (the descriptor's pointers are tested for NULL and alignment only):
 *   70000 + 1000 NPL + 100 NH + 10 MODE + 2 CTX + SIDE
 * NPL = 3 (USF_PLANES_BF16X3) or 2 (USF_PLANES_F16X2), NH = n_hidden, MODE = 0 inference / 1 hidden_out / 2 USF_ACT_GATE; the code
 * comes from the very branches that launch.  0 for M == 0; the negative value the launch would return for a descriptor it
 * rejects (usf_last_error set). */
int usf_coupling_planes_variant(const usf_coupling_planes_desc* d, int32_t has_ctx, int32_t has_side);

/* The backward twin of usf_gated_norm_rows_f32 (usflows_hip.h; ABI 34): what torch.autograd derives from GatedMLP's gate (networks.py:222-245) and LayerNormVector
 * (:206-219) in Flow.fit, rows of [M, C] fp32, r / mean / variance recomputed from (skip, vg) as the forward computes them:
 *     g = dy * gamma;  dr = (g - mean_c g - xh * mean_c(g xh)) / sqrt(var r + eps)        (gamma == NULL: dr = dy)
 *     d_skip = dr;  d_vg[:, :C] = dr * sigmoid(gate);  d_vg[:, gate_off:] = dr * val * sigmoid(gate) (1 - sigmoid(gate))
 *     dy_xh = dy * xh  (optional, needs gamma: dgamma = its column sums, dbeta = the column sums of dy -- usf_colsum_f32)
 * Columns [C, c_pad) of every output are written as zeros (operand padding of the GEMMs that follow); gate_off >= c_pad. */
typedef struct usf_gated_norm_bwd_desc {
  const float* skip;   int64_t ld_skip;
  const float* vg;     int64_t ld_vg;    int64_t gate_off;
  const float* gamma;
  const float* dy;     int64_t ld_dy;
  float*       d_skip; int64_t ld_d_skip;
  float*       d_vg;   int64_t ld_d_vg;
  float*       dy_xh;  int64_t ld_dy_xh;
  int64_t M, C, c_pad;
  float eps, reserved;
} usf_gated_norm_bwd_desc;
int usf_gated_norm_rows_bwd_f32(const usf_gated_norm_bwd_desc* d, usf_stream_t stream);

/* The last step of LUTransform's parameter gradients under Flow.fit (what autograd derives through transforms.py:1271-1320's
 * tril(L_raw, -1) + I and triu(U_raw), and the log-det term sum log|diag U|), for n blocks at once, fp64 in / fp32 out:
 *     dL_out[i] = tril(dL[i] (+ TL[i]), -1)                     dU_out[i] = triu(dU[i] (+ TU[i])) + diag(c[i] / diag(U_i))
 * dL / dU [n, D, D]: the chain-rule products (only the wanted triangle has to be valid); TL / TU: the products of the M = L U
 * usages, or NULL; c [n]: coefficient of the log-det term; tri [2n, D, D] as usf_lu_prepare_f64 leaves it (U_i^T at 2i + 1).
 * One pass instead of triu / tril / diagonal add / sums / converting copies over [n, D, D] tensors. */
int usf_lu_grad_finish_f64(const double* dL, const double* dU, const double* TL, const double* TU, const double* c,
                           const double* tri, int64_t n, int64_t D, float* dL_out, float* dU_out, usf_stream_t stream);

/*
 * ---- backward pass of the training step -----------------------------------------------
 * Flow.fit (flows.py:196-199) differentiates -log_prob(batch).mean(); these are the batch-sized pieces of that
 * backward pass (usf_train.hip).  Data gradients of the linear layers are usf_linear_f32 launches on the transposed
 * weight image (usf_pack_weight_f32 with transpose = 1).
 *
 * usf_wgrad_f32: G[n,k] = alpha * sum_m Y[m,n] * A[m,k] + beta * G[n,k]   -- the weight gradient of F.linear
 *   (Y = gradient at the layer's output [M,N], A = the layer's input [M,K]); exact-f32 MFMA, the batch is cut into
 *   row ranges whose partial products are summed in a fixed order (bitwise reproducible).  Y / A rows must be 16-byte
 *   aligned (ld % 4 == 0).  workspace: at least usf_wgrad_workspace_floats(M,N,K) floats.  mode 0: exact-f32 MFMA;
 *   mode 1: the bf16x3 split of DESIGN.md 3.1b (fp32-equivalent accuracy on the bf16 matrix cores; used from M >= 2048;
 *   from 8192 rows with enough output tiles to fill the chip, and while (M + 448) * max(ldy, lda) * 4 < 2^32, the
 *   loader-wave kernel: it reads Y / A with 8-byte buffer loads bounded by the end of the row extent ((M-1) * ld + N resp.
 *   K floats from the base pointer) -- the same memory the contract above names; with an odd N or K the pair that holds
 *   the last column of row M - 1 straddles that bound and the hardware still returns its in-range half (the bound is
 *   checked per dword: measured, tests/test_wgrad_kernels_gpu.py).  Rows >= M are never read; columns [N, ld) / [K, ld)
 *   of rows < M may be read and only reach outputs that are not stored (a NaN there is harmless).  A row range may come
 *   out EMPTY (usf_wgrad_plan): its partial image is all zeros.  The workspace need be no larger than reported.
 * usf_wgrad_variant: which kernel such a call launches -- 0 exact-f32, 1 bf16x3 (256 threads), 2 bf16x3 with loader
 *   waves (introspection for the parity tests).
 * usf_colsum_f32: out[n] = alpha * sum_m Y[m,n] + beta * out[n]           -- the bias gradient; workspace
 *   (ceil(M/256) + ceil(M/65536) + 2) * N floats (partials of the 256-row levels).
 */
int usf_wgrad_f32(const float* Y, int64_t ldy, const float* A, int64_t lda, int64_t M, int64_t N, int64_t K, float* G,
                  int64_t ldg, float alpha, float beta, int32_t mode, float* workspace, int64_t workspace_floats,
                  usf_stream_t stream);
int64_t usf_wgrad_workspace_floats(int64_t M, int64_t N, int64_t K);
int usf_wgrad_variant(int64_t M, int64_t N, int64_t K, int64_t ldy, int64_t lda, int32_t mode);
/* usf_wgrad_plan (an addition: USF_INTERNAL_VERSION is unchanged; host only, launches nothing, needs no GPU): what a
 * usf_wgrad_f32 (with_colsum = 0) or usf_wgrad_bias_f32 (with_colsum = 1) call of these sizes launches, answered from the code
 * the call itself launches from (introspection for the parity tests).  Writes 8 values and returns 8 (cap >= 8), < 0 on bad
 * arguments or where usf_wgrad_bias_ok refuses the column sums:
 *   out[0] usf_wgrad_variant, out[1] row ranges, out[2] rows per range (a multiple of 32; the last range may be shorter, or
 *   EMPTY -- its partial image is then all zeros), out[3] 1: one range written straight to G, no reduction launch,
 *   out[4] grid blocks (tiles * row ranges rounded up to 8; surplus blocks leave at once), out[5] threads per block,
 *   out[6] 1: a reduction launch follows, out[7] the workspace floats the call insists on (never more than
 *   usf_wgrad_workspace_floats). */
int usf_wgrad_plan(int64_t M, int64_t N, int64_t K, int64_t ldy, int64_t lda, int32_t mode, int32_t with_colsum, int64_t* out,
                   int32_t cap);
/* usf_wgrad_f32 and the layer's bias gradient in one pass (ABI 32): colsum_out[n] = cs_alpha * sum_m Y[m,n] + cs_beta *
 * colsum_out[n] (what usf_colsum_f32 computes), from the operand fragments the bf16x3 kernels hold anyway -- three more
 * MFMAs per fragment row against an operand of ones in the blocks of tile column 0; partial sums in a fixed order.  Only
 * where usf_wgrad_bias_ok says 1 (usf_wgrad_variant >= 1, i.e. mode 1 from 2048 rows, and K >= 64); the same workspace
 * as usf_wgrad_f32. */
int usf_wgrad_bias_f32(const float* Y, int64_t ldy, const float* A, int64_t lda, int64_t M, int64_t N, int64_t K, float* G,
                       int64_t ldg, float alpha, float beta, int32_t mode, float* colsum_out, float cs_alpha, float cs_beta,
                       float* workspace, int64_t workspace_floats, usf_stream_t stream);
int usf_wgrad_bias_ok(int64_t M, int64_t N, int64_t K, int64_t ldy, int64_t lda, int32_t mode);
int usf_colsum_f32(const float* Y, int64_t ldy, int64_t M, int64_t N, float* out, float alpha, float beta,
                   float* workspace, int64_t workspace_floats, usf_stream_t stream);

/*
 * The weight gradient from PRE-SPLIT operands (ABI 32).  usf_wgrad_f32's loader waves split every fp32 operand value
 * into its three bf16 planes again in each of the blocks that share its rows (seven times at 784 x 784); here Y and A
 * arrive as the planes the layer's own GEMMs already made of them (usf_linear_desc::A_planes_out: the forward GEMM
 * splits the layer input, the data-gradient GEMM the output gradient), or as usf_split_planes_f32 writes them:
 *   plane p of an operand at base + p * plane_stride elements, each [ceil32(M), ld] bf16 row-major, ld % 8 == 0,
 *   plane_stride % 8 == 0, plane_stride >= ceil32(M) * ld, 16-byte aligned base, rows [M, ceil32(M)) zero,
 *   the three planes of one operand below 4 GiB; x == p0 + p1 + p2 (round-to-nearest residual split) -- bit for bit for
 *   2^-110 <= |x| < 2^127 and for zeros (measured on the device, both load paths, tests/test_wgrad_kernels_gpu.py): below
 *   2^-110 the third plane's bits fall under bf16's smallest subnormal 2^-133 and are rounded there (an error of at most
 *   2^-134, absolute); from 2^127 a mantissa above 1.fe rounds the first plane to infinity.  Gradients and activations of
 *   the training path lie inside the range or are flushed to it without harm (an absolute error of 2^-134 per value).
 * usf_wgrad_planes_f32: G[n,k] = alpha * sum_m Y[m, y_off + n] * A[m, a_off + k] + beta * G[n,k]  (y_off, a_off % 8 == 0)
 *   -- the same six products per value pair in the same order as usf_wgrad_f32 mode 1, one block per CU over row ranges
 *   of equal length, partial sums added in a fixed order (bitwise reproducible).  workspace: at least
 *   usf_wgrad_planes_workspace_floats(M, N, K) floats.  usf_wgrad_planes_ok: 1 where the kernel pays (the loader-wave
 *   kernel's cross-over: M >= 8192 and enough tiles), else 0 -- callers then keep usf_wgrad_f32.
 *   colsum_out (may be NULL; needs usf_wgrad_planes_colsum_ok = K >= 64): colsum_out[n] = cs_alpha * sum_m Y[m, y_off + n]
 *   + cs_beta * colsum_out[n] -- the layer's bias gradient (usf_colsum_f32) from the fragments the kernel holds anyway:
 *   three more MFMAs per fragment row against an operand of ones in the blocks of tile column 0.
 * usf_split_planes_f32: P[p][m][c] for m < ceil32(M), c < ldp: the planes of X[m, c] (zeros for m >= M or c >= N).
 * Replaces: the weight-gradient half of autograd's F.linear backward (flows.py:196-203, transforms.py:913-962,
 * networks.py:739-751) at training batches of thousands of rows.
 */
int usf_wgrad_planes_f32(const void* Y_planes, int64_t ldyp, int64_t y_plane_stride, int64_t y_off, const void* A_planes,
                         int64_t ldap, int64_t a_plane_stride, int64_t a_off, int64_t M, int64_t N, int64_t K, float* G,
                         int64_t ldg, float alpha, float beta, float* colsum_out, float cs_alpha, float cs_beta, float* workspace,
                         int64_t workspace_floats, usf_stream_t stream);
int64_t usf_wgrad_planes_workspace_floats(int64_t M, int64_t N, int64_t K);
int usf_wgrad_planes_ok(int64_t M, int64_t N, int64_t K);
int usf_wgrad_planes_colsum_ok(int64_t M, int64_t N, int64_t K);
/* usf_wgrad_planes_plan (an addition: USF_INTERNAL_VERSION is unchanged; host only, launches nothing): the schedule a
 * usf_wgrad_planes_f32 / usf_wgrad_blocked_f32 call with this workspace launches from, chosen by the code the calls choose with.
 * workspace_floats < 0: the size usf_wgrad_planes_workspace_floats reports.  cus > 0: that many compute units instead of the
 * device's (no GPU needed, as in usf_conv_wgrad_wide_variant); cus = 0: the device's.  Tile classes c = 3 * (type in n) + (type
 * in k), types 0 normal (128 wide), 1 wide (128 + a folded remainder of up to 16), 2 edge (the remainder alone); class 4 does not
 * exist.  Writes 35 values and returns 35 (cap >= 35), < 0 on bad arguments / no schedule:
 *   out[0] 1 balanced, 0 plain grid; out[1], out[2] the remainder of N, of K rides in the last normal tile; out[3] grid blocks;
 *   out[4] items; out[5] the workspace floats the call insists on (with_colsum: the partial column sums included); out[6] partial
 *   images; out[7 + c] tiles, out[16 + c] row ranges (= partials), out[25 + c] rows per range of class c; out[34] the workspace
 *   the answer assumed. */
int usf_wgrad_planes_plan(int64_t M, int64_t N, int64_t K, int64_t workspace_floats, int32_t with_colsum, int32_t cus, int64_t* out,
                          int32_t cap);
int usf_split_planes_f32(const float* X, int64_t ldx, int64_t M, int64_t N, void* planes, int64_t ldp, int64_t plane_stride,
                         usf_stream_t stream);
/* The same weight gradient with both operands in the BLOCKED planes format of the planes pipeline (ABI 33) -- the buffers the
 * training forward's usf_gemm_planes_bf16x3 / usf_coupling_planes launches leave behind and the backward's launches write:
 *   G[n,k] = alpha * sum_m Y[m, 32 y_kb0 + n] * A[m, 32 a_kb0 + k] + beta * G[n,k],   n < N, k < K  (LOGICAL positions),
 * Y / A planes buffers of ceil(M/16) panels with y_nkb / a_nkb blocks per panel (USF_PLANES_BF16X3), N <= 32 (y_nkb - y_kb0),
 * K <= 32 (a_nkb - a_kb0).  Rows [M, 16 ceil(M/16)) of Y must hold zeros (they do in every buffer whose producer chain
 * starts at usf_pack_planes_f32 and has no bias); those of A must be finite.  Same kernel, schedule, order of products,
 * workspace (usf_wgrad_planes_workspace_floats) and colsum_out semantics as usf_wgrad_planes_f32; a buffer must stay below
 * 2 GiB.  Loader waves copy whole 1-KiB chunks; the MFMA waves' transposing reads un-do the slot order, so G comes out in
 * logical order. */
int usf_wgrad_blocked_f32(const void* Y_planes, int64_t y_nkb, int64_t y_kb0, const void* A_planes, int64_t a_nkb, int64_t a_kb0,
                          int64_t M, int64_t N, int64_t K, float* G, int64_t ldg, float alpha, float beta, float* colsum_out,
                          float cs_alpha, float cs_beta, float* workspace, int64_t workspace_floats, usf_stream_t stream);
/* The reduction of usf_wgrad_blocked_f32 queued (round 5; large-batch training: 129 weight gradients per step end with a reduction of
 * ~18 us each, one after the other although only the parameter update waits for them).  usf_wgrad_blocked_plan_f32 = the same call
 * that launches the multiply kernel only and fills *job (HOST memory): G / colsum_out stay unwritten and the workspace stays in use
 * until a usf_wgrad_reduce_jobs_f32 launch containing the job has run (jobs / block_job DEVICE arrays as for
 * usf_partial_sum_jobs_f32: job j owns the blocks [first_block, first_block + blocks), first_block set by the caller).  Same
 * additions in the same order as the undeferred call: same bits. */
typedef struct usf_wreduce_job {
  const float* part; float* out; const float* cs_part; float* cs_out;
  int64_t rows, cols, ldo;
  float alpha, beta, cs_alpha, cs_beta;
  int32_t first_block, blocks;
  unsigned char sched[64];                      /* the schedule's tile classes (opaque) */
} usf_wreduce_job;
int usf_wgrad_blocked_plan_f32(const void* Y_planes, int64_t y_nkb, int64_t y_kb0, const void* A_planes, int64_t a_nkb, int64_t a_kb0,
                          int64_t M, int64_t N, int64_t K, float* G, int64_t ldg, float alpha, float beta, float* colsum_out,
                          float cs_alpha, float cs_beta, float* workspace, int64_t workspace_floats, usf_wreduce_job* job, usf_stream_t stream);
int usf_wgrad_reduce_jobs_f32(const usf_wreduce_job* jobs, const int32_t* block_job, int64_t n_blocks, usf_stream_t stream);

/* Many small weight / bias gradients in ONE launch.  At the reference's training batch (32 rows, tests/explib/mnist.yaml:34)
 * Flow.fit's backward pass (flows.py:196-199) asks for one weight and one bias gradient per F.linear on the path -- some
 * hundreds of launches of a few microseconds whose dispatch, not their work, bounds the step.  `jobs` is a DEVICE array;
 * `block_job` a DEVICE array with the job index of every block of the launch (n_blocks entries; job j owns the blocks
 * first_block .. first_block + its own count - 1, in order):
 *   A != NULL: G[n,k] = alpha * sum_m Y[m,n] A[m,k] + beta * G[n,k], ceil(N/128) * ceil(K/128) blocks, exact-f32 MFMA over
 *              one row range -- bit-identical to usf_wgrad_f32 (mode 0) on the same operands for M <= 256; the alignment
 *              rules of usf_wgrad_f32 apply;
 *   A == NULL: G[n] = alpha * sum_m Y[m,n] + beta * G[n], ceil(N/64) blocks (fixed summation order: reproducible).
 * Meant for M <= 256; jobs of one launch must not write what another job of the same launch reads or writes. */
typedef struct usf_grad_job {
  const float* Y;
  const float* A;
  float* G;
  int64_t ldy, lda, ldg;
  int32_t M, N, K, first_block;
  float alpha, beta;
} usf_grad_job;
int usf_grad_jobs_f32(const usf_grad_job* jobs, const int32_t* block_job, int64_t n_blocks, usf_stream_t stream);

/*
 * SophiaG over all parameter tensors of a model in one launch (sophia.py:39-58 update_hessian, 151-199
 * _single_tensor_sophiag -- the optimiser Flow.fit defaults to, flows.py:116).  `chunks` is a DEVICE array; a chunk is
 * one block's share (any length; the host side cuts tensors into pieces of 16 384 elements) of one fp32 parameter
 * tensor p with its gradient g, momentum m (exp_avg) and Hessian estimate h.
 *   usf_sophiag_step_f32:    p *= decay (= 1 - lr * weight_decay);  m = m * beta1 + g * one_minus_beta1 (g negated with
 *                            maximize);  ratio = min(|m| / (rho_bs * h + 1e-15), 1) (rho_bs = rho * bs);
 *                            p += neg_lr * sign(m) * ratio
 *   usf_sophiag_hessian_f32: h = h * beta2 + one_minus_beta2 * g * g
 */
typedef struct usf_mt_chunk {
  float* p; const float* g; float* m; float* h;
  int32_t n; int32_t reserved;
} usf_mt_chunk;
int usf_sophiag_step_f32(const usf_mt_chunk* chunks, int64_t n_chunks, float decay, float beta1, float one_minus_beta1,
                         float rho_bs, float neg_lr, int32_t maximize, usf_stream_t stream);
int usf_sophiag_hessian_f32(const usf_mt_chunk* chunks, int64_t n_chunks, float beta2, float one_minus_beta2,
                            usf_stream_t stream);

/*
 * Adam / AdamW (torch/optim/adam.py, _single_tensor_adam, the non-capturable branch) over all fp32 tensors of a parameter
 * group in one launch, in torch's operation order:
 *   g' = maximize ? -g : g;   L2 decay: g' = fma(wd, p, g');   decoupled decay (AdamW): p *= 1 - lr * wd
 *   m = lerp(m, g', 1 - beta1);   v = v * beta2 + (1 - beta2) * g' * g';   amsgrad: vmax = max(vmax, v)
 *   denom = sqrt(v | vmax) / sqrt(1 - beta2^t) + eps;   p += (-lr / (1 - beta1^t)) * (m / denom)
 * `chunks` is a DEVICE array, one 256-thread block per chunk (the host cuts tensors into pieces of 16 384 elements); vmax
 * is read with USF_ADAM_AMSGRAD only.  The step count t lives on the DEVICE: steps[n_slots] (int64), one counter per group
 * of tensors that have taken the same number of steps; a chunk names its counter in `slot`.  The call first adds 1 to
 * every counter in a small launch of its own, then runs the update, whose blocks only read them -- so a captured call
 * (hipGraph) advances t on every replay.  beta^t is computed in fp64 on the device, everything else in fp32.  No
 * atomics, no host read-back.  28 bytes of HBM traffic per parameter and step (36 with amsgrad).
 */
typedef struct usf_adam_chunk {
  float* p; const float* g; float* m; float* v; float* vmax;
  int32_t n; int32_t slot;
} usf_adam_chunk;
#define USF_ADAM_MAXIMIZE 1
#define USF_ADAM_AMSGRAD 2
#define USF_ADAM_DECOUPLED 4
int usf_adam_step_f32(const usf_adam_chunk* chunks, int64_t n_chunks, int64_t* steps, int64_t n_slots, double lr, double beta1,
                      double beta2, double eps, double weight_decay, int32_t flags, usf_stream_t stream);

/*
 * torch.nn.utils.clip_grad_norm_(params, max_norm) with the 2-norm and error_if_nonfinite=False, over a DEVICE table of
 * gradient chunks, without atomics or a host synchronisation:
 *   usf_grad_sqnorm_partials_f32: partials[b] = the sum of squares of chunk b in fp64 (one block per chunk, fixed order)
 *   usf_grad_clip_scale_f32:      every block adds all n_chunks partials in one fixed order, forms
 *                                 coef = min(max_norm / (sqrt(total) + 1e-6), 1) (fp64, rounded to fp32 once) and scales
 *                                 its chunk of g in place.  A non-finite norm propagates as in torch.
 */
typedef struct usf_grad_chunk {
  float* g;
  int32_t n; int32_t reserved;
} usf_grad_chunk;
int usf_grad_sqnorm_partials_f32(const usf_grad_chunk* chunks, int64_t n_chunks, double* partials, usf_stream_t stream);
int usf_grad_clip_scale_f32(const usf_grad_chunk* chunks, int64_t n_chunks, const double* partials, double max_norm,
                            usf_stream_t stream);

/* (Leaky)ReLU backward from the saved layer OUTPUT h: d[m,j] *= (h[m,j] > 0 ? 1 : slope), slope >= 0
 * (ATen leaky_relu_backward on the pre-activation; sign(h) == sign(pre-activation)). networks.py:745-749 */
int usf_act_grad_f32(float* d, int64_t ldd, const float* h, int64_t ldh, int64_t M, int64_t H, int32_t act, float slope,
                     usf_stream_t stream);

/* Backward of usf_base_logprob_f32: g[m,d] = g_lp[m] * d/dz base_d(z[m,d]) for d < D, 0 for D <= d < ldg
 * (flows.py:245 through torch Laplace.log_prob / Normal.log_prob).  For the LPNORM* ids g_lp is the gradient at the
 * radius r[m] = ||z[m,:] - loc||_p (RadialDistribution.log_prob, distributions.py:501-505) and `scale` carries that
 * radius vector [M] (the forward kernel's output). */
int usf_base_logprob_grad_f32(const float* z, int64_t ldz, const float* g_lp, int64_t M, int64_t D, int32_t base,
                              const float* loc, const float* scale, float* g, int64_t ldg, usf_stream_t stream);

/*
 * The backward of usf_affine_prep_f32 (usflows_hip.h), same operands:
 * usf_affine_prep_bwd_f32: from the forward pass's Minv and b and (dM, dMinv, db, dc, dladj) -- zeros where an output was
 * not used -- the gradients of the
 * parameters: dL_raw (strictly lower triangle, zeros elsewhere: the reference's gradient mask, transforms.py:1262-1268),
 * dU_raw (upper triangle), dbias [n, C], dvk [n, nvs, C].  What autograd derives from the reference's matrix() /
 * inverse_matrix() / bias() / log_abs_det_jacobian() chains, in two launches instead of some hundreds.
 */
int usf_affine_prep_bwd_f32(const float* save, const float* bias, const float* vk, const float* w0, const float* Minv,
                            const float* b, const float* dM, const float* dMinv, const float* db, const float* dc,
                            const float* dladj, int64_t n, int32_t C, int32_t nvs, float* dL_raw, float* dU_raw, float* dbias,
                            float* dvk, usf_stream_t stream);

/* Trainable Laplace / Normal base (the reference's distributions.Laplace / Normal modules, distributions.py:199-238, as a flow's
 * base distribution under Flow.fit, flows.py:196-203) -- ABI 33:
 *   d_loc_scale[d]     = sum_m g_lp[m] * d/dloc_d   base_d(z[m,d]; loc_d, scale_d)
 *   d_loc_scale[D + d] = sum_m g_lp[m] * d/dscale_d base_d(...)          (scale = the CONSTRAINED scale the density uses;
 * the caller applies softplus' for the modules' scale_unconstrained).  Laplace: sign(t)/b, |t|/b^2 - 1/b; Normal: t/s^2,
 * t^2/s^3 - 1/s (t = z - loc).  Row ranges of 256 summed in a fixed order (bit-reproducible).  workspace: at least
 * (ceil(M/256) + ceil(M/65536) + 4) * 2 D floats. */
int usf_base_param_grad_f32(const float* z, int64_t ldz, const float* g_lp, int64_t M, int64_t D, int32_t base, const float* loc,
                            const float* scale, float* d_loc_scale, float* workspace, int64_t workspace_floats, usf_stream_t stream);

/* Measurement aid (bench.py: roofline.sustained_peak): ONE launch of a register-only loop of the planes GEMM's matrix-core
 * instruction mix (v_mfma_f32_16x16x32_bf16, 10 x 2 accumulator tiles, six products per fp32-equivalent product; 512 threads,
 * two waves per SIMD; no LDS, no memory traffic in the loop) -- `iters` slabs of 120 MFMAs per wave on `blocks` blocks
 * (0: two per CU).  src1024: 1024 finite floats (device); sink: one float (device, never written); *flops_out (host, may be
 * NULL): the bf16 MFMA flops of the launch (fp32-equivalent: / 6).  The caller times the launch with events on `stream`. */
int usf_mfma_probe(const float* src1024, float* sink, int64_t iters, int64_t blocks, double* flops_out, usf_stream_t stream);
/* Measurement aid (bench.py: roofline.clock_mhz): while dev_buf2 (device memory, two 64-bit counters, zeroed by the caller) is
 * set, every block of usf_gemm_planes_bf16x3's kernel and of usf_mfma_probe adds its lifetime to it -- [0] in shader-clock cycles
 * (s_memtime), [1] in ticks of the constant 100 MHz counter (s_memrealtime): 100 MHz x [0] / [1] is the clock the matrix cores ran
 * at under that kernel (the nominal peaks assume 2400 MHz).  NULL: off (the default; the kernels then read no counter).
 * One process-wide setting (not per device, not synchronised with launches in flight): set it, launch, synchronise, clear it. */
int usf_set_clock_buffer(unsigned long long* dev_buf2);

/* Tuning knobs of the kernels' host code (A/B switches, cross-overs): named integers, preset on first use from the environment
 * variable USFLOWS_AMD_TUNE ("name=value,..."), changed at run time here.  usf_get_tuning(name, dflt): the value in force. */
int usf_set_tuning(const char* name, int64_t value);
int64_t usf_get_tuning(const char* name, int64_t dflt);

#ifdef __cplusplus
}
#endif
#endif /* USFLOWS_HIP_INTERNAL_H */
