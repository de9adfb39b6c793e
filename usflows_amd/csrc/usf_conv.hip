// Convolution conditioner of the image-shaped flows: Conv2d with stride 1, "same" zero padding,
// kernel 1 x 1, 3 x 3, 4 x 4 or 5 x 5 (networks.py:405-510 ConvNet2D, :61-122 GatedConv; 4 x 4 / 5 x 5 where the taps' weight planes
// and two samples fit the LDS, otherwise on the streamed kernel of usf_conv_stream.hip) as an implicit GEMM on the bf16 matrix cores
// with the fp32-equivalent bf16x3 arithmetic of the rest of the path (three bf16 planes per operand, six
// v_mfma_f32_16x16x32_bf16 per product, fp32 accumulation).
//
//   y[b, co, p] = out_act( bias[co] + sum_{tap, ci} W[co, ci, tap] * a[b, ci, p + tap] ),   a = in_act(x) * in_mul
//
// in_act: the (Leaky)ReLU GatedConv / ConvNet2D put in front of a convolution; in_mul [Cin * H * W]: the coupling mask
// of MaskedCoupling (x * mask feeds the first convolution); both fold into the staging pass.
//
// Data flow of a 512-thread block (persistent over groups of S samples):
//   * weights: pre-split planes [3][CoutP][KP] bf16 (K order: tap-major, channel-minor, channels padded to Cp = ceil8(Cin),
//     KP = ceil32(taps * Cp)) copied into LDS once per block;
//   * inputs: the S samples of a group are read from HBM once (coalesced fp32), activated / masked, split into three bf16
//     planes and written into a zero-bordered LDS image [S x (H+2)(W+2) positions][Cp channels] -- channel-minor, so a
//     lane's MFMA operand (8 consecutive k = 8 channels of one tap) is one 16-byte LDS read at position (p + tap);
//   * GEMM: M = output channels (A operand = weights), N = rows (sample, pixel) of the group (B operand = input image),
//     K = taps * Cp; a wave owns 32 x 32 output patches (2 x 2 MFMA tiles: every fragment read feeds 12 MFMAs);
//   * epilogue: bias, activation, 16 consecutive pixels per store instruction.
// Row strides of both LDS images are an odd number of 16-byte units: the 16 lanes of a fragment read hit 16 different
// bank groups.
#include "usf_common.h"
#include "usf_conv_plan.h"
#include <type_traits>

namespace usf {

typedef __bf16 cv_bf16x8 __attribute__((ext_vector_type(8)));

struct ConvArgs {
  const float* x; float* y;
  const __bf16* wp;            // [3][coutp][kp]
  const float* bias;           // [cout] or null
  const float* in_mul;         // [cin * hw] or null
  int B, cin, cout, H, W, ks;
  int cp, kp, coutp;           // padded channel count, padded K, padded Cout (multiple of 16)
  int S;                       // samples per group
  int xs16, ws16;              // LDS row strides in 16-byte units (odd)
  int in_act, out_act; float in_slope, out_slope;
  const float* gate_x; int gateC;   // gated mode (GatedConv's second convolution + its gate): see usf_conv2d_same_f32
  int dbg;                     // tuning aid (USF_CONV_DBG): 1 no staging, 2 no k loop, 4 no output stores, 8 no input loads
  const float* ctx; int ctx_stride;   // context channel (CTX instantiation only): ctx[b * ctx_stride], see usf_conv2d_same_ctx_f32
  const float* w_ctx;          // [cout][ks * ks] weights of the context channel
  int pb;                      // K4 instantiations only: zeros before the image in each axis, 1 (torch's "same") or 2 (its mirror image)
};

__device__ __forceinline__ void cv_split(float x, __bf16& h, __bf16& m, __bf16& l) {
  h = (__bf16)x;
  const float r = x - (float)h;
  m = (__bf16)r;
  l = (__bf16)(r - (float)m);
}

// CTX: the context channel's rank-1 term joins the bias in the epilogue (usf_conv2d_same_ctx_f32); false: the plain kernel
// K5: the ks = 5 instantiations (their context mask is ctx_tapmask5); false: ks = 1 / 3, compiled as before ks = 5 existed
// K4: the ks = 4 instantiations: the padded image is (H + 3) x (W + 3), a.pb of its zeros lie before the image; context mask ctx_tapmask4
template <bool CTX, bool K5 = false, bool K4 = false>
__global__ __launch_bounds__(512, 2) void conv2d_same_bf16x3_kernel(const ConvArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int li = lane & 15, lg = lane >> 4;
  const int HW = a.H * a.W;
  const int pad = K4 ? a.pb : a.ks >> 1;
  const int PW = K4 ? a.W + 3 : a.W + 2 * pad, PP = (K4 ? a.H + 3 : a.H + 2 * pad) * PW;   // padded image
  const int taps = a.ks * a.ks;
  const int wrow = a.ws16 * 16, xrow = a.xs16 * 16;                // bytes per LDS row
  const int wplane = a.coutp * wrow, xplane = a.S * PP * xrow;      // bytes per plane
  unsigned char* const Wl = smem;
  unsigned char* const Xl = smem + 3 * wplane;

  // ---- once per block: weights into LDS, the input image zeroed (borders and padding channels stay zero) ----
  {
    const int units = a.kp / 8;                                      // 16-byte units per weight row
    for (int i = tid; i < 3 * a.coutp * units; i += 512) {
      const int pl = i / (a.coutp * units), rem = i % (a.coutp * units);
      const int r = rem / units, u = rem % units;
      *reinterpret_cast<cv_bf16x8*>(Wl + pl * wplane + r * wrow + u * 16) =
          *reinterpret_cast<const cv_bf16x8*>(a.wp + ((size_t)(pl * a.coutp + r) * a.kp + 8 * u));
    }
    const f32x4 z = {0.f, 0.f, 0.f, 0.f};
    for (int i = tid; i < 3 * xplane / 16; i += 512) *reinterpret_cast<f32x4*>(Xl + i * 16) = z;
  }
  __syncthreads();

  const int ngroups = (a.B + a.S - 1) / a.S;
  const int nblk = a.kp / 32;
  const int cpairs = (a.cin + 1) >> 1;
  const int ppass = (HW + 63) >> 6;                                  // 64-pixel passes over a channel plane
  // Staging: a wave takes (sample, channel pair) planes, a lane one pixel of both channels -- two coalesced loads, two
  // splits, three 4-byte LDS stores (the pair is adjacent in the channel-minor image).  The loads of group g + 1 are
  // issued before the MFMA phase of group g and consumed after it: HBM latency hides under the matrix work.
  constexpr int MAXIT = 16;                                          // (host: S is chosen so that a group needs <= MAXIT)
  float pre[MAXIT][2];
  // per 64-pixel pass q: this lane's pixel and the LDS offset of its (padded) position -- no divisions in the loops below
  int poff[4], pix[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int p = min(lane + 64 * q, HW - 1);
    const int py = p / a.W, px = p - py * a.W;
    pix[q] = (lane + 64 * q < HW) ? p : -1;
    poff[q] = ((py + pad) * PW + (px + pad)) * xrow;
  }
  auto fetch = [&](int gidx) {
    const int s0 = gidx * a.S;
    const int npl = min(a.S, a.B - s0) * cpairs;                      // (sample, channel pair) planes of the group
    const float* xg = a.x + (size_t)s0 * a.cin * HW;
    int j = 0, q = 0;                                                 // plane round / pixel pass of iteration `it` (wave-uniform)
#pragma unroll
    for (int it = 0; it < MAXIT; ++it) {
      const int pp = wave + 8 * j;
      const int p = q == 0 ? pix[0] : q == 1 ? pix[1] : q == 2 ? pix[2] : pix[3];
      pre[it][0] = pre[it][1] = 0.f;
      if (pp < npl && p >= 0) {
        const int sl = pp / cpairs, c = 2 * (pp - sl * cpairs);
        const float* x0 = xg + ((size_t)sl * a.cin + c) * HW + p;
        pre[it][0] = x0[0];
        if (c + 1 < a.cin) pre[it][1] = x0[HW];
      }
      if (++q == ppass) { q = 0; ++j; }
    }
  };
  auto stage = [&](int gidx) {
    const int s0 = gidx * a.S;
    const int npl = min(a.S, a.B - s0) * cpairs;
    int j = 0, q = 0;
#pragma unroll
    for (int it = 0; it < MAXIT; ++it) {
      const int pp = wave + 8 * j;
      const int p = q == 0 ? pix[0] : q == 1 ? pix[1] : q == 2 ? pix[2] : pix[3];
      const int po = q == 0 ? poff[0] : q == 1 ? poff[1] : q == 2 ? poff[2] : poff[3];
      if (pp < npl && p >= 0) {
        const int sl = pp / cpairs, c = 2 * (pp - sl * cpairs);
        float v0 = act_apply(pre[it][0], a.in_act, a.in_slope), v1 = act_apply(pre[it][1], a.in_act, a.in_slope);
        if (a.in_mul) {
          v0 *= a.in_mul[c * HW + p];
          if (c + 1 < a.cin) v1 *= a.in_mul[(c + 1) * HW + p];
        }
        __bf16 h0, m0, l0, h1, m1, l1;
        cv_split(v0, h0, m0, l0);
        cv_split(v1, h1, m1, l1);
        unsigned char* dst = Xl + sl * PP * xrow + po + 2 * c;
        typedef __bf16 bf2 __attribute__((ext_vector_type(2)));
        *reinterpret_cast<bf2*>(dst) = (bf2){h0, h1};
        *reinterpret_cast<bf2*>(dst + xplane) = (bf2){m0, m1};
        *reinterpret_cast<bf2*>(dst + 2 * xplane) = (bf2){l0, l1};
      }
      if (++q == ppass) { q = 0; ++j; }
    }
  };
  if ((int)blockIdx.x < ngroups) fetch(blockIdx.x);
  for (int gidx = blockIdx.x; gidx < ngroups; gidx += gridDim.x) {
    const int s0 = gidx * a.S;
    const int ns = min(a.S, a.B - s0);
    const int R = ns * HW;                                           // live rows of this group
    if (!(a.dbg & 1)) stage(gidx);
    __syncthreads();
    if (gidx + (int)gridDim.x < ngroups && !(a.dbg & 8)) fetch(gidx + gridDim.x);
    // ---- implicit GEMM: 32 (co) x 32 (rows) patches dealt over the waves ----
    // Patch shape by the amount of work in the group: 32 (co) x 32 (rows) when that gives every wave a patch, otherwise
    // 16 x 32 or 16 x 16 (more patches, fewer MFMAs per fragment read)
    auto patches = [&](auto pc_, auto pr_) {
      constexpr int PC = decltype(pc_)::value, PR = decltype(pr_)::value;      // 16-row tiles per patch in co / rows
      const int ctn = (a.coutp / 16 + PC - 1) / PC, rtn = (R + 16 * PR - 1) / (16 * PR);
      for (int t = wave; t < ctn * rtn; t += 8) {
        const int ct = t / rtn, rt = t - ct * rtn;
        // this lane's row positions (B operand columns): row r -> (sample, pixel) -> top-left of its window
        int xbase[PR];
#pragma unroll
        for (int b = 0; b < PR; ++b) {
          const int r = min(rt * 16 * PR + b * 16 + li, R - 1);
          const int sl = r / HW, p = r - sl * HW;
          const int py = p / a.W, px = p - py * a.W;
          xbase[b] = (sl * PP + py * PW + px) * xrow;
        }
        const int co0 = ct * 16 * PC;
        const bool two_co = PC == 2 && co0 + 16 < a.coutp;              // wave-uniform
        int wbase[PC];
        wbase[0] = (co0 + li) * wrow;
        if (PC == 2) wbase[PC - 1] = (min(co0 + 16, a.coutp - 16) + li) * wrow;
        f32x4 acc[PC][PR];
#pragma unroll
        for (int i = 0; i < PC; ++i)
#pragma unroll
          for (int b = 0; b < PR; ++b) acc[i][b] = (f32x4){0.f, 0.f, 0.f, 0.f};
        cv_bf16x8 wf[2][PC][3], xf[2][PR][3];                            // [buffer][tile][plane]: block k + 1 is read under block k
        auto read_blk = [&](int blk, cv_bf16x8 (&w)[PC][3], cv_bf16x8 (&xv)[PR][3]) {
          const int kflat = blk * 32 + 8 * lg;
          int tap = kflat / a.cp;
          const int c = kflat - tap * a.cp;
          tap = min(tap, taps - 1);                                      // K padding: weights are zero there
          const int dy = tap / a.ks, dx = tap - dy * a.ks;
          const int xoff = (dy * PW + dx) * xrow + 2 * c;
          const int woff = 2 * kflat;
#pragma unroll
          for (int pl = 0; pl < 3; ++pl) {
#pragma unroll
            for (int i = 0; i < PC; ++i) w[i][pl] = *reinterpret_cast<const cv_bf16x8*>(Wl + pl * wplane + wbase[i] + woff);
#pragma unroll
            for (int b = 0; b < PR; ++b) xv[b][pl] = *reinterpret_cast<const cv_bf16x8*>(Xl + pl * xplane + xbase[b] + xoff);
          }
        };
        auto mm_blk = [&](const cv_bf16x8 (&w)[PC][3], const cv_bf16x8 (&xv)[PR][3]) {
#define USF_CV(I, B_, P, Q) acc[I][B_] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w[I][P], xv[B_][Q], acc[I][B_], 0, 0, 0)
#pragma unroll
          for (int b = 0; b < PR; ++b) {
            USF_CV(0, b, 2, 0); USF_CV(0, b, 1, 1); USF_CV(0, b, 0, 2); USF_CV(0, b, 1, 0); USF_CV(0, b, 0, 1); USF_CV(0, b, 0, 0);
            if (PC == 2 && two_co) {
              USF_CV(PC - 1, b, 2, 0); USF_CV(PC - 1, b, 1, 1); USF_CV(PC - 1, b, 0, 2); USF_CV(PC - 1, b, 1, 0); USF_CV(PC - 1, b, 0, 1);
              USF_CV(PC - 1, b, 0, 0);
            }
          }
#undef USF_CV
        };
        read_blk(0, wf[0], xf[0]);
        int blk = (a.dbg & 2) ? nblk : 0;
        for (; blk + 2 <= nblk; blk += 2) {
          read_blk(blk + 1, wf[1], xf[1]);
          mm_blk(wf[0], xf[0]);
          read_blk(min(blk + 2, nblk - 1), wf[0], xf[0]);
          mm_blk(wf[1], xf[1]);
        }
        if (blk < nblk) mm_blk(wf[0], xf[0]);
        // ---- epilogue: lane (col = li, g = lg) of tile (i, b) holds output channels co0 + 16 i + 4 g + (0..3) of row b*16 + li
#pragma unroll
        for (int b = 0; b < PR; ++b) {
          const int r = rt * 16 * PR + b * 16 + li;
          if (r >= R) continue;
          const int sl = r / HW, p = r - sl * HW;
          float* yb = a.y + ((size_t)(s0 + sl) * a.cout) * HW + p;
          float cx = 0.f;
          unsigned cmask = 0u;
          if constexpr (CTX) {
            const int py = p / a.W;
            cx = a.ctx[(size_t)(s0 + sl) * a.ctx_stride];
            cmask = K4 ? ctx_tapmask4(py, p - py * a.W, a.H, a.W)
                       : K5 ? ctx_tapmask5(py, p - py * a.W, a.H, a.W) : ctx_tapmask(py, p - py * a.W, a.H, a.W, a.ks);
          }
          if (PC == 2 && a.gateC > 0) {
            // gated mode: the patch's two tiles are (value, gate) of the same 16 channels (rows interleaved at pack time):
            // y[c] = x[c] + value * sigmoid(gate) -- GatedConv.forward's tail (networks.py:108-122) without the [B, 2C] tensor
            const size_t gb = ((size_t)(s0 + sl) * a.gateC) * HW + p;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
              const int c = (co0 >> 1) + 4 * lg + j;
              if (c < a.gateC && !(a.dbg & 4)) {
                const float val = acc[0][b][j] + (a.bias ? a.bias[co0 + 4 * lg + j] : 0.f);
                const float gt = acc[PC - 1][b][j] + (a.bias ? a.bias[co0 + 16 + 4 * lg + j] : 0.f);
                a.y[gb + (size_t)c * HW] = a.gate_x[gb + (size_t)c * HW] + val * (1.f / (1.f + expf(-gt)));
              }
            }
            continue;
          }
#pragma unroll
          for (int i = 0; i < PC; ++i) {
            if (i == 1 && !two_co) break;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
              const int co = co0 + 16 * i + 4 * lg + j;
              if (co < a.cout && !(a.dbg & 4)) {
                float v = acc[i][b][j] + (a.bias ? a.bias[co] : 0.f);
                if constexpr (CTX) v += cx * ctx_tapsum(a.w_ctx + co * taps, taps, cmask);
                yb[(size_t)co * HW] = act_apply(v, a.out_act, a.out_slope);
              }
            }
          }
        }
      }
    };
    typedef std::integral_constant<int, 1> I1;
    typedef std::integral_constant<int, 2> I2;
    const int shape = conv_patch_shape(a.coutp, R, a.gateC);         // (usf_conv_plan.h: the probe reports the same rule)
    if (shape == 0x22) patches(I2(), I2());
    else if (shape == 0x21) patches(I2(), I1());                     // (value, gate) tile pairs stay together
    else if (shape == 0x12) patches(I1(), I2());
    else patches(I1(), I1());
    __syncthreads();                                                 // the image is rewritten by the next group
  }
}

// second kernel (usf_conv_wreg.hip): 1 = launched, 0 = shape not served there, < 0 = error
int conv2d_same_wreg(const float* x, float* y, int64_t B, int64_t cin, int64_t cout, int64_t H, int64_t W, const void* wplanes,
                     const float* bias, const float* in_mul, int32_t in_act, float in_slope, int32_t out_act, float out_slope,
                     const float* res_x, const float* res_mul, float res_sign, int res_mode, hipStream_t stream,
                     const float* ctx = nullptr, int64_t ctx_stride = 0, const float* w_ctx = nullptr);

static int odd16(int units) { return units | 1; }
// fourth kernel (usf_conv_stream.hip)
int conv2d_same_stream(const float* x, float* y, int64_t B, int64_t cin, int64_t cout, int64_t H, int64_t W, const void* wplanes,
                       const float* bias, const float* in_mul, int32_t in_act, float in_slope, int32_t out_act, float out_slope,
                       const float* ctx, int64_t ctx_stride, const float* w_ctx, const ConvSPlan& pl, hipStream_t stream, int ks = 5,
                       int pad_before = 2);

// LDS bytes of a launch with S samples per group; the layout the kernel derives from the same numbers
static int64_t conv_lds_bytes(int cin, int cout, int H, int W, int ks, int S, int* xs16, int* ws16, int* cp_, int* kp_, int* coutp_) {
  const int cp = (cin + 7) / 8 * 8, taps = ks * ks, kp = (taps * cp + 31) / 32 * 32, coutp = (cout + 15) / 16 * 16;
  const int PP = (H + ks - 1) * (W + ks - 1);                       // (ks = 4: three zeros per axis, in either placement)
  *xs16 = odd16(cp / 8); *ws16 = odd16(kp / 8); *cp_ = cp; *kp_ = kp; *coutp_ = coutp;
  return 3LL * coutp * (*ws16) * 16 + 3LL * S * PP * (*xs16) * 16;
}

// elements ([3][coutp][kp] bf16) of the weight planes usf_conv2d_same_f32 expects for these sizes
int64_t conv2d_weight_elems(int64_t cin, int64_t cout, int64_t ks) {
  if (cin <= 0 || cout <= 0 || (ks != 1 && ks != 3 && ks != 4 && ks != 5)) return -1;
  const int64_t cp = (cin + 7) / 8 * 8, kp = (ks * ks * cp + 31) / 32 * 32, coutp = (cout + 15) / 16 * 16;
  return 3 * coutp * kp;
}

static int conv_k45_route(int cin, int cout, int H, int W, int ks, bool gated, int* S_best);

// samples per group the kernel would use for these sizes (the LDS decides); 0: the shape is not served
int conv2d_same_fits(int64_t cin, int64_t cout, int64_t H, int64_t W, int64_t ks) {
  if (cin <= 0 || cout <= 0 || H <= 0 || W <= 0 || cin > 64 || cout > 64 || H * W > 256 || (ks != 1 && ks != 3 && ks != 4 && ks != 5)) return 0;
  if (ks == 4 || ks == 5) {
    int S = 0;
    return conv_k45_route((int)cin, (int)cout, (int)H, (int)W, (int)ks, false, &S) ? S : 0;
  }
  int xs, ws, cp, kp, coutp;
  for (int S = 8; S >= 1; --S)
    if (conv_lds_bytes((int)cin, (int)cout, (int)H, (int)W, (int)ks, S, &xs, &ws, &cp, &kp, &coutp) <= 158 * 1024 &&
        conv_stage_iters((int)cin, (int)(H * W), S) <= 16) return S;
  return 0;
}

// The first kernel's launch for B samples of a shape conv2d_same accepts: as many samples per group as fit 158 KB of LDS and
// the staging registers (at most 8; at least one has to fit: else -3 with p->lds = one sample's bytes), clipped to B; one
// block per group up to the device's compute units (cus == 0: ask the device).
int conv_first_plan(int64_t B, int cin, int cout, int H, int W, int ks, int cus, ConvPlan* p) {
  int S = 8;
  int64_t lds = 0;
  for (; S >= 1; --S) {
    lds = conv_lds_bytes(cin, cout, H, W, ks, S, &p->xs16, &p->ws16, &p->cp, &p->kp, &p->coutp);
    if (lds <= 158 * 1024 && conv_stage_iters(cin, H * W, S) <= 16) break;
  }
  p->lds = lds;
  p->S = S < 1 ? 0 : S;
  p->groups = 0; p->grid = 0;
  if (S < 1) return -3;
  if (S > B) {
    S = (int)B;
    lds = conv_lds_bytes(cin, cout, H, W, ks, S, &p->xs16, &p->ws16, &p->cp, &p->kp, &p->coutp);
  }
  p->S = S; p->lds = lds;
  if (cus <= 0) cus = device_cu_count();
  p->groups = (B + S - 1) / S;
  p->grid = (unsigned)(p->groups < cus ? p->groups : cus);
  return 0;
}

// ks = 4 / 5: the first kernel where its weights and two samples fit the LDS, otherwise the streamed kernel (no gated mode
// there), otherwise the first kernel with one sample.  Neither plan looks at the placement of a 4 x 4 kernel's zeros.
static int conv_k45_route(int cin, int cout, int H, int W, int ks, bool gated, int* S_best) {
  ConvPlan p1;
  const int s1 = conv_first_plan(1 << 20, cin, cout, H, W, ks, 1, &p1) == 0 ? p1.S : 0;
  ConvSPlan ps;
  const int ss = gated ? 0 : (conv_stream_plan(1 << 20, cin, cout, H, W, 1, &ps, ks) == 0 ? ps.S : 0);
  if (s1 >= 2 || ss < 1) { *S_best = s1; return s1 >= 1 ? 1 : 0; }
  *S_best = ss;
  return 4;
}
int conv_k5_route(int cin, int cout, int H, int W, bool gated, int* S_best) { return conv_k45_route(cin, cout, H, W, 5, gated, S_best); }
int conv_k4_route(int cin, int cout, int H, int W, bool gated, int* S_best) { return conv_k45_route(cin, cout, H, W, 4, gated, S_best); }

// usf_conv2d_same_variant: the plans above, asked instead of launched (no pointer is looked at, nothing is launched)
int conv2d_same_variant(const usf_conv_variant_query* q, usf_conv_variant* o) {
  if (!q || !o) { set_error("usf_conv2d_same_variant: null pointer"); return -1; }
  *o = usf_conv_variant();
  o->max_mHW = o->max_mW = o->max_mSE = o->max_mSO = -1;
  const int64_t B = q->B, cin = q->cin, cout = q->cout, H = q->H, W = q->W, ks = q->ks;
  const int e = q->entry;
  if (e < USF_CONV_ENTRY_PLAIN || e > USF_CONV_ENTRY_GATED) { set_error("usf_conv2d_same_variant: bad entry"); return -2; }
  if (B <= 0 || cin <= 0 || cout <= 0 || H <= 0 || W <= 0 || B > 0x7fffffff) return 0;
  const bool fused = e == USF_CONV_ENTRY_RES || e == USF_CONV_ENTRY_GATE_MUL || e == USF_CONV_ENTRY_GATE_ADD;
  const bool first_ok = !(cin > 64 || cout > 64 || H * W > 256 || (ks != 1 && ks != 3 && ks != 4 && ks != 5));   // conv2d_same's size rule
  if (fused ? ks != 3 : !first_ok) return 0;
  if (e == USF_CONV_ENTRY_GATED && cout % 32 != 0) return 0;
  const int cus = q->cus > 0 ? q->cus : device_cu_count();
  if (ks == 3 && e != USF_CONV_ENTRY_GATED) {
    ConvWQuery wq;
    wq.B = B; wq.cin = cin; wq.cout = cout; wq.H = H; wq.W = W;
    wq.aligned = q->aligned != 0;
    wq.has_res = fused; wq.res_mul = fused; wq.res_alias = false;
    wq.res_mode = e == USF_CONV_ENTRY_GATE_MUL ? 1 : (e == USF_CONV_ENTRY_GATE_ADD ? 2 : 0);
    wq.cus = cus;
    ConvWPlan wp;
    conv_wreg_launch_plan(wq, &wp);
    if (wp.kernel) {
      o->kernel = wp.kernel; o->S = wp.S; o->grid = wp.grid; o->groups = wp.groups; o->lds_bytes = wp.lds;
      o->NB = wp.NB; o->CP = wp.CP; o->NCT = wp.NCT; o->CTX = e == USF_CONV_ENTRY_CTX;
      o->max_mHW = wp.max_mHW; o->max_mW = wp.max_mW; o->max_mSE = wp.max_mSE; o->max_mSO = wp.max_mSO;
      return 0;
    }
  }
  if (fused) return 0;                                     // the fused forms live on the second / third kernel only
  if (ks == 4 || ks == 5) {
    int sb = 0;
    const int route = conv_k45_route((int)cin, (int)cout, (int)H, (int)W, (int)ks, e == USF_CONV_ENTRY_GATED, &sb);
    if (route == 0) return 0;
    if (route == 4) {
      ConvSPlan sp;
      if (conv_stream_plan(B, (int)cin, (int)cout, (int)H, (int)W, cus, &sp, (int)ks) != 0) return 0;
      o->kernel = 4; o->S = sp.S; o->grid = sp.grid; o->groups = sp.groups; o->lds_bytes = sp.lds;
      o->NB = sp.KS / 32; o->CP = sp.cp; o->NCT = sp.depth; o->CTX = e == USF_CONV_ENTRY_CTX;
      o->PC_full = o->PC_last = 2; o->PR_full = o->PR_last = sp.NR;
      return 0;
    }
  }
  ConvPlan p;
  if (conv_first_plan(B, (int)cin, (int)cout, (int)H, (int)W, (int)ks, cus, &p) != 0) return 0;
  o->kernel = 1; o->S = p.S; o->grid = p.grid; o->groups = p.groups; o->lds_bytes = p.lds;
  o->CTX = e == USF_CONV_ENTRY_CTX;
  const int gateC = e == USF_CONV_ENTRY_GATED ? 1 : 0, HW = (int)(H * W);
  const int full = conv_patch_shape(p.coutp, p.S * HW, gateC);
  const int last = conv_patch_shape(p.coutp, (int)(B - (p.groups - 1) * p.S) * HW, gateC);
  o->PC_full = full >> 4; o->PR_full = full & 15; o->PC_last = last >> 4; o->PR_last = last & 15;
  return 0;
}

int conv2d_same(const float* x, float* y, int64_t B, int64_t cin, int64_t cout, int64_t H, int64_t W, int64_t ks,
                const void* wplanes, const float* bias, const float* in_mul, int32_t in_act, float in_slope,
                int32_t out_act, float out_slope, const float* gate_x, int64_t gate_channels, hipStream_t stream,
                const float* ctx, int64_t ctx_stride, const float* w_ctx, int pad_before) {
  if (pad_before < 0) pad_before = (int)((ks - 1) / 2);             // the public entry points: torch's "same" placement
  if (B < 0 || cin <= 0 || cout <= 0 || H <= 0 || W <= 0 || cin > 64 || cout > 64 || H * W > 256 || (ks != 1 && ks != 3 && ks != 4 && ks != 5) ||
      B > 0x7fffffff) {
    set_error("usf_conv2d_same_f32: unsupported sizes (channels 1..64, H * W <= 256, kernel 1, 3, 4 or 5)");
    return -2;
  }
  if (pad_before != (ks - 1) / 2 && pad_before != ks / 2) {
    set_error("usf_conv2d_same_pad_f32: pad_before must be (ks - 1) / 2 or, at an even ks, ks / 2");
    return -2;
  }
  if (pad_before != (ks - 1) / 2 && (ctx || gate_x)) {
    set_error("usf_conv2d_same_pad_f32: the mirrored placement has no context or gated form");
    return -2;
  }
  if (B == 0) return 0;
  if (!x || !y || !wplanes) { set_error("usf_conv2d_same_f32: null pointer"); return -1; }
  if (x == y) { set_error("usf_conv2d_same_f32: in-place operation is not supported"); return -2; }
  if ((gate_x != nullptr) != (gate_channels > 0) || (gate_x && (cout != 32 * ((gate_channels + 15) / 16) || out_act != USF_ACT_NONE))) {
    set_error("usf_conv2d_same_f32: gated mode wants gate_x, gate_channels C > 0, cout = 32 * ceil(C / 16) interleaved rows, no output activation");
    return -2;
  }
  if (!aligned16(wplanes)) { set_error("usf_conv2d_same_f32: weight planes must be 16-byte aligned"); return -2; }
  for (int32_t act : {in_act, out_act})
    if (act != USF_ACT_NONE && act != USF_ACT_LEAKY_RELU) { set_error("usf_conv2d_same_f32: bad act"); return -2; }
  if (ctx && (!w_ctx || gate_x || (ctx_stride != 0 && ctx_stride != 1))) {
    set_error("usf_conv2d_same_ctx_f32: the context channel wants w_ctx, ctx_stride 0 or 1 and no gated mode");
    return -2;
  }
  if (ks == 3 && !gate_x) {
    // the register-weight kernel where it serves the shape (the conditioner layers of the reference's image configurations)
    const int rc = conv2d_same_wreg(x, y, B, cin, cout, H, W, wplanes, bias, in_mul, in_act, in_slope, out_act, out_slope, nullptr,
                                    nullptr, 0.f, 0, stream, ctx, ctx_stride, w_ctx);
    if (rc != 0) return rc < 0 ? rc : 0;
  }
  if (ks == 4 || ks == 5) {
    int sb = 0;
    const int route = conv_k45_route((int)cin, (int)cout, (int)H, (int)W, (int)ks, gate_x != nullptr, &sb);
    if (route == 4) {
      ConvSPlan sp;
      if (conv_stream_plan(B, (int)cin, (int)cout, (int)H, (int)W, 0, &sp, (int)ks) != 0) {
        set_error("usf_conv2d_same_f32: no streamed plan");
        return -3;
      }
      return conv2d_same_stream(x, y, B, cin, cout, H, W, wplanes, bias, in_mul, in_act, in_slope, out_act, out_slope, ctx, ctx_stride,
                                w_ctx, sp, stream, (int)ks, pad_before);
    }
  }
  ConvArgs a;
  a.x = x; a.y = y; a.wp = reinterpret_cast<const __bf16*>(wplanes); a.bias = bias; a.in_mul = in_mul;
  a.B = (int)B; a.cin = (int)cin; a.cout = (int)cout; a.H = (int)H; a.W = (int)W; a.ks = (int)ks;
  a.in_act = in_act; a.out_act = out_act; a.in_slope = in_slope; a.out_slope = out_slope;
  a.dbg = (int)tuning("conv_dbg", 0);
  a.gate_x = gate_x; a.gateC = (int)gate_channels;
  a.ctx = ctx; a.ctx_stride = (int)ctx_stride; a.w_ctx = w_ctx;
  a.pb = pad_before;
  ConvPlan pl;
  if (conv_first_plan(B, a.cin, a.cout, a.H, a.W, a.ks, 0, &pl) != 0) {
    set_error("usf_conv2d_same_f32: one sample does not fit the LDS / staging registers (%lld bytes)", (long long)pl.lds);
    return -3;
  }
  const int64_t lds = pl.lds;
  a.xs16 = pl.xs16; a.ws16 = pl.ws16; a.cp = pl.cp; a.kp = pl.kp; a.coutp = pl.coutp;
  a.S = pl.S;
  static bool attr_done_dev[6][USF_MAX_DEVICES] = {{false}};   // (the attribute belongs to the device and the instantiation)
  const bool k5 = ks == 5, k4 = ks == 4;
  bool& attr_done = attr_done_dev[(ctx ? 1 : 0) + (k5 ? 2 : 0) + (k4 ? 4 : 0)][current_device_slot()];
  const void* kfn = k4 ? (ctx ? reinterpret_cast<const void*>(&conv2d_same_bf16x3_kernel<true, false, true>)
                              : reinterpret_cast<const void*>(&conv2d_same_bf16x3_kernel<false, false, true>))
                  : k5 ? (ctx ? reinterpret_cast<const void*>(&conv2d_same_bf16x3_kernel<true, true>)
                              : reinterpret_cast<const void*>(&conv2d_same_bf16x3_kernel<false, true>))
                       : (ctx ? reinterpret_cast<const void*>(&conv2d_same_bf16x3_kernel<true>)
                              : reinterpret_cast<const void*>(&conv2d_same_bf16x3_kernel<false>));
  if (!attr_done) {
    if (hipFuncSetAttribute(kfn, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024) != hipSuccess) {
      set_error("usf_conv2d_same_f32: cannot raise the LDS limit");
      return -4;
    }
    attr_done = true;
  }
  const unsigned grid = pl.grid;
  if (k4 && ctx) hipLaunchKernelGGL((conv2d_same_bf16x3_kernel<true, false, true>), dim3(grid), dim3(512), (size_t)lds, stream, a);
  else if (k4) hipLaunchKernelGGL((conv2d_same_bf16x3_kernel<false, false, true>), dim3(grid), dim3(512), (size_t)lds, stream, a);
  else if (k5 && ctx) hipLaunchKernelGGL((conv2d_same_bf16x3_kernel<true, true>), dim3(grid), dim3(512), (size_t)lds, stream, a);
  else if (k5) hipLaunchKernelGGL((conv2d_same_bf16x3_kernel<false, true>), dim3(grid), dim3(512), (size_t)lds, stream, a);
  else if (ctx) hipLaunchKernelGGL(conv2d_same_bf16x3_kernel<true>, dim3(grid), dim3(512), (size_t)lds, stream, a);
  else hipLaunchKernelGGL(conv2d_same_bf16x3_kernel<false>, dim3(grid), dim3(512), (size_t)lds, stream, a);
  return check_launch(ctx ? "usf_conv2d_same_ctx_f32" : "usf_conv2d_same_f32");
}

// y = res_x + res_sign * (res_mul * conv(...)): the last convolution of a coupling's conditioner with MaskedCoupling's
// residual in its output stream.  Only where the register-weight kernel serves the shape: 0 = done, 1 = not served here (the
// caller runs the convolution and usf_masked_residual_f32 as two passes), < 0 = error.
int conv2d_same_res(const float* x, float* y, int64_t B, int64_t cin, int64_t cout, int64_t H, int64_t W, int64_t ks,
                    const void* wplanes, const float* bias, const float* in_mul, int32_t in_act, float in_slope,
                    const float* res_x, const float* res_mul, float res_sign, hipStream_t stream) {
  if (B < 0 || cin <= 0 || cout <= 0 || H <= 0 || W <= 0 || B > 0x7fffffff) { set_error("usf_conv2d_same_res_f32: bad sizes"); return -2; }
  if (B == 0) return 0;
  if (!x || !y || !wplanes || !res_x || !res_mul) { set_error("usf_conv2d_same_res_f32: null pointer"); return -1; }
  if (x == y || res_x == y) { set_error("usf_conv2d_same_res_f32: in-place operation is not supported"); return -2; }
  if (in_act != USF_ACT_NONE && in_act != USF_ACT_LEAKY_RELU) { set_error("usf_conv2d_same_res_f32: bad act"); return -2; }
  if (ks != 3) return 1;
  const int rc = conv2d_same_wreg(x, y, B, cin, cout, H, W, wplanes, bias, in_mul, in_act, in_slope, USF_ACT_NONE, 0.f, res_x, res_mul,
                                  res_sign, 0, stream);
  return rc < 0 ? rc : (rc == 1 ? 0 : 1);
}

// y = conv(x) * (gate_h > 0 ? 1 : gate_slope) * gate_mul: a data-gradient convolution with the (Leaky)ReLU and mask factors
// of the layer's INPUT in its output stream (what usf_act_grad_f32 and a mask product would do in two more passes).
// 0 = done, 1 = not served here, < 0 = error.
int conv2d_same_gate(const float* x, float* y, int64_t B, int64_t cin, int64_t cout, int64_t H, int64_t W, int64_t ks,
                     const void* wplanes, const float* gate_h, float gate_slope, const float* gate_mul, const float* gate_add,
                     hipStream_t stream) {
  if (B < 0 || cin <= 0 || cout <= 0 || H <= 0 || W <= 0 || B > 0x7fffffff) { set_error("usf_conv2d_same_gate_f32: bad sizes"); return -2; }
  if (B == 0) return 0;
  if (!x || !y || !wplanes || !gate_h) { set_error("usf_conv2d_same_gate_f32: null pointer"); return -1; }
  if (x == y || gate_h == y) { set_error("usf_conv2d_same_gate_f32: in-place operation is not supported"); return -2; }
  if (ks != 3) return 1;
  if (gate_add && gate_mul) { set_error("usf_conv2d_same_gate_f32: gate_mul and gate_add exclude each other"); return -2; }
  if (gate_add == y) { set_error("usf_conv2d_same_gate_f32: in-place operation is not supported"); return -2; }
  const int rc = conv2d_same_wreg(x, y, B, cin, cout, H, W, wplanes, nullptr, nullptr, USF_ACT_NONE, 0.f, USF_ACT_NONE, 0.f, gate_h,
                                  gate_add ? gate_add : gate_mul, gate_slope, gate_add ? 2 : 1, stream);
  return rc < 0 ? rc : (rc == 1 ? 0 : 1);
}

}  // namespace usf
