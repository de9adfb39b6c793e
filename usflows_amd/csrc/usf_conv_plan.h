// Launch plans of the "same" convolution's three kernels (usf_conv.hip, usf_conv_wreg.hip): ONE statement of which kernel
// serves a call, with how many samples per group, on how many blocks and with which LDS layout.  The entry points launch
// from these plans and usf_conv2d_same_variant (usflows_hip_internal.h) answers from them: the probe cannot drift from
// the launch path.  Host code but for conv_patch_shape, which the first kernel evaluates per group.
#ifndef USF_CONV_PLAN_H
#define USF_CONV_PLAN_H
#include <stdint.h>

namespace usf {

// Patch shape of conv2d_same_bf16x3_kernel for a group of R live rows: (PC << 4) | PR, PC / PR = 16-row tiles per patch in
// output channels / rows.  32 x 32 when that gives every wave a patch, otherwise 16 x 32 or 16 x 16 (more patches, fewer
// MFMAs per fragment read); gated mode keeps the (value, gate) tile pairs together: 32 x 32 or 32 x 16.
__host__ __device__ inline int conv_patch_shape(int coutp, int R, int gateC) {
  const int c16 = coutp / 16, r32 = (R + 31) / 32;
  if (((c16 + 1) / 2) * r32 >= 7 || (gateC > 0 && (c16 / 2) * r32 >= 4)) return 0x22;
  if (gateC > 0) return 0x21;
  if (c16 * r32 >= 7) return 0x12;
  return 0x11;
}

// first kernel (conv2d_same_bf16x3_kernel)
struct ConvPlan {
  int S;                        // samples per group (0: not even one sample fits)
  int64_t lds;                  // dynamic LDS bytes of the launch
  int xs16, ws16, cp, kp, coutp;
  int64_t groups;
  unsigned grid;
};

// second and third kernel (conv2d_same_wreg_kernel / conv2d_same_wsp_kernel)
struct ConvWPlan {
  int kernel;                   // 0: not served here (the caller uses the first kernel / two passes), 2 register-weight, 3 wave-specialised
  int S, cgs, img_bytes;
  int64_t lds;
  int64_t groups;
  unsigned grid;
  int NB, CP, NCT;              // the instantiation
  unsigned mHW, mW, mSE, mSO;   // floor(2^32 / d) + 1 for d = H W, W, cin H W, cout H W
  int max_mHW, max_mW, max_mSE, max_mSO;   // largest n the kernel divides with each of them (-1: that division is not made)
};

// what of a call decides the plan of the second / third kernel
struct ConvWQuery {
  int64_t B, cin, cout, H, W;
  bool aligned;                 // x, y, in_mul, res_x, res_mul (those given) are 16-byte aligned
  bool has_res;                 // res_x given (residual, gate-mul or gate-add form)
  bool res_mul;                 // res_mul given
  int res_mode;                 // 0 residual, 1 gate-mul, 2 gate-add
  bool res_alias;               // res_x == y
  int cus;                      // compute units to plan for
};

// fourth kernel (conv2d_same_stream_kernel, usf_conv_stream.hip): 5 x 5 and 4 x 4, weights streamed through an LDS ring
struct ConvSPlan {
  int S;                        // samples per group, clipped to B (0: not even one sample fits)
  int S_best;                   // ... of a batch that does not clip it
  int KS, depth, nslab;         // K values per slab (64 / 32), slabs in the ring (2), slabs per walk
  int NR;                       // the instantiation: 16-row tiles per wave (1, 2, 4)
  int64_t lds;
  int xs16, ss16, cp, kp, coutp;
  int64_t groups;
  unsigned grid;
};

// fifth kernel (conv2d_same_band_kernel, usf_conv_band.hip): ks = 1 / 3 on maps of up to 4096 pixels, a group = a band of rows
struct ConvBPlan {
  int RB;                       // output rows per band of this launch (0: not served)
  int RB_best;                  // ... the shape's own band, before the caller's cap
  int nbands, last_rows;        // bands per sample, output rows of a sample's last band
  int iters, npass;             // register-staged iterations per thread, 64-pixel passes over a full band's staged rows
  int64_t lds, wbytes;          // dynamic LDS bytes of the launch, of which the weight planes
  int xs16, ws16, cp, kp, coutp;
  int64_t groups;               // B * nbands
  unsigned grid;
};
// register-staged iterations per thread for a band whose image has `rows` rows (output rows + ks - 1) of W pixels
inline int conv_band_stage_iters(int cin, int W, int rows) { return (((cin + 1) / 2 + 7) / 8) * ((rows * W + 63) / 64); }
// 0: *p is the launch plan; 1: the shape is not served (p->RB_best / p->wbytes are still filled where the sizes are in range)
int conv_band_plan(int64_t B, int64_t cin, int64_t cout, int64_t H, int64_t W, int64_t ks, int band_rows, int cus, ConvBPlan* p);

// register-staged iterations per thread for a group of S samples (the first and fourth kernel hold at most 16 pixel pairs per thread)
inline int conv_stage_iters(int cin, int HW, int S) { return ((S * ((cin + 1) / 2) + 7) / 8) * ((HW + 63) / 64); }

int conv_first_plan(int64_t B, int cin, int cout, int H, int W, int ks, int cus, ConvPlan* p);
int conv_stream_plan(int64_t B, int cin, int cout, int H, int W, int cus, ConvSPlan* p, int ks = 5);
// which kernel serves ks = 5 for these sizes: 1 (weights resident: its best S >= 2, or nothing else fits), 4 (streamed), 0 (none);
// *S_best = samples per group of a batch that does not clip them
int conv_k5_route(int cin, int cout, int H, int W, bool gated, int* S_best);
// the same rule for ks = 4; one answer serves both placements of its zeros (1 before / 2 after, and the mirror image): the padded
// image is (H + 3) x (W + 3) either way
int conv_k4_route(int cin, int cout, int H, int W, bool gated, int* S_best);
void conv_wreg_launch_plan(const ConvWQuery& q, ConvWPlan* p);

}  // namespace usf
#endif
