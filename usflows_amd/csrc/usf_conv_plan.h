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

int conv_first_plan(int64_t B, int cin, int cout, int H, int W, int ks, int cus, ConvPlan* p);
void conv_wreg_launch_plan(const ConvWQuery& q, ConvWPlan* p);

}  // namespace usf
#endif
