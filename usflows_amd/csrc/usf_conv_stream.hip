// Fourth kernel of the "same" convolution: 5 x 5 taps with the weights STREAMED (usf_conv2d_same_f32 / _ctx_f32 at ks = 5 where
// the first kernel cannot keep three weight planes of 25 taps and two padded samples in the LDS: 32 -> 32 channels alone is
// 155 136 B of planes), and the 4 x 4 instantiations of the same kernel (KSZ = 4: 16 taps, K = 16 cp is a whole number of
// slabs; a (H + 3) x (W + 3) image with a.pb zeros before it in each axis -- 1: torch's "same", 2: its mirror image).
// Operands, K order and arithmetic are the first kernel's (usf_conv.hip): planes [3][coutp][kp] bf16,
// tap-major / channel-minor K, six v_mfma_f32_16x16x32_bf16 per product, fp32 accumulation, in_act / in_mul / bias / out_act.
//
// Data flow of a 512-thread block (persistent over groups of S samples):
//   * inputs: the group's padded image [S x (H+4)(W+4) positions][cp channels] x 3 planes stays in the LDS for the whole K
//     walk (staged as the first kernel stages it; the next group's loads are issued before the walk and consumed after it);
//   * weights: K slabs of KS = 64 or 32 values (at cp = 64 a tap / half a tap) x coutp rows x 3 planes move through a ring of
//     two LDS buffers.  Slab s + 1 is loaded from global memory into registers BEFORE the barrier of slab s, the MFMAs of
//     slab s run, then the registers are written into the other buffer: ONE barrier per slab -- a wave that has passed the
//     barrier of slab s has finished reading slab s - 1, whose buffer slab s + 1 overwrites.  The ring runs on across groups
//     (slab 0 of the next group is loaded under the last slab of this one; its buffer is (slabs so far) & 1);
//   * GEMM: every wave keeps its accumulators over the whole walk: output tiles (2 x 16 channels) x (NR x 16 rows); the
//     8 waves split into ceil(coutp / 32) channel groups times 8 / that many row ranges;
//   * epilogue: the first kernel's (bias, context term, activation).
// Row strides of both LDS images are an odd number of 16-byte units, as in the first kernel.
#include "usf_common.h"
#include "usf_conv_plan.h"

namespace usf {

typedef __bf16 cs_bf16x8 __attribute__((ext_vector_type(8)));

struct ConvSArgs {
  const float* x; float* y;
  const __bf16* wp;            // [3][coutp][kp]
  const float* bias;           // [cout] or null
  const float* in_mul;         // [cin * hw] or null
  int B, cin, cout, H, W;
  int cp, kp, coutp;
  int S;                       // samples per group
  int xs16, ss16;              // LDS row strides (image / slab) in 16-byte units (odd)
  int KS, nslab;               // K values per slab, slabs per walk
  unsigned mcp;                // floor(2^20 / cp) + 1: k / cp == (k * mcp) >> 20 for k < 2^14
  int in_act, out_act; float in_slope, out_slope;
  const float* ctx; int ctx_stride;
  const float* w_ctx;          // [cout][KSZ * KSZ]
};
// the 4 x 4 instantiations' arguments: the placement behind the 5 x 5 ones' (whose kernel arguments stay what they were)
struct ConvSArgs4 : ConvSArgs {
  int pb;                      // zeros before the image in each axis (1: torch's "same", 2: its mirror image)
};
template <int KSZ> struct ConvSArgsOf { typedef ConvSArgs type; };
template <> struct ConvSArgsOf<4> { typedef ConvSArgs4 type; };

__device__ __forceinline__ void cs_split(float x, __bf16& h, __bf16& m, __bf16& l) {
  h = (__bf16)x;
  const float r = x - (float)h;
  m = (__bf16)r;
  l = (__bf16)(r - (float)m);
}

template <int NR, bool CTX, int KSZ>
__global__ __launch_bounds__(512) void conv2d_same_stream_kernel(const typename ConvSArgsOf<KSZ>::type a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  static_assert(KSZ == 4 || KSZ == 5, "5 x 5 or 4 x 4");
  constexpr int TAPS = KSZ * KSZ;
  int PAD = 2;                                                       // (a constant of the 5 x 5 instantiations)
  if constexpr (KSZ == 4) PAD = a.pb;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int li = lane & 15, lg = lane >> 4;
  const int HW = a.H * a.W;
  constexpr int PADT = KSZ - 1;                                      // zeros per axis, before and after
  const int PW = a.W + PADT, PP = (a.H + PADT) * PW;                 // padded image
  const int xrow = a.xs16 * 16, srow = a.ss16 * 16;                  // bytes per LDS row
  const int xplane = a.S * PP * xrow, splane = a.coutp * srow;       // bytes per plane
  unsigned char* const Xl = smem;
  unsigned char* const Rl = smem + 3 * xplane;                       // ring [2][3][coutp][srow]

  // ---- the slab mover: this thread's (plane, row, 16-byte unit) of a full slab, up to three of them ----
  constexpr int WU = 3;                                              // (host: 3 * coutp * KS / 8 <= 3 * 512)
  int wsrc[WU], wdst[WU], wk[WU];
  {
    const int ku = a.KS >> 3, per = a.coutp * ku;
#pragma unroll
    for (int j = 0; j < WU; ++j) {
      const int i = tid + 512 * j;
      const int pl = i / per, rem = i - pl * per;
      const int r = rem / ku, u = rem - r * ku;
      wsrc[j] = (pl * a.coutp + r) * a.kp + 8 * u;
      wdst[j] = pl * splane + r * srow + 16 * u;
      wk[j] = i < 3 * per ? 8 * u : (1 << 30);                       // (the last slab may be short: k >= kp is not moved)
    }
  }
  cs_bf16x8 wreg[WU];
  auto wload = [&](int s) {
#pragma unroll
    for (int j = 0; j < WU; ++j)
      if (s * a.KS + wk[j] < a.kp) wreg[j] = *reinterpret_cast<const cs_bf16x8*>(a.wp + wsrc[j] + s * a.KS);
  };
  auto wstore = [&](int s, int buf) {
#pragma unroll
    for (int j = 0; j < WU; ++j)
      if (s * a.KS + wk[j] < a.kp) *reinterpret_cast<cs_bf16x8*>(Rl + buf * 3 * splane + wdst[j]) = wreg[j];
  };

  // ---- once per block: the input image zeroed (borders and padding channels stay zero) ----
  {
    const f32x4 z = {0.f, 0.f, 0.f, 0.f};
    for (int i = tid; i < 3 * xplane / 16; i += 512) *reinterpret_cast<f32x4*>(Xl + i * 16) = z;
  }
  __syncthreads();

  const int ngroups = (a.B + a.S - 1) / a.S;
  const int cpairs = (a.cin + 1) >> 1;
  const int ppass = (HW + 63) >> 6;                                  // 64-pixel passes over a channel plane
  // Staging as in the first kernel: a wave takes (sample, channel pair) planes, a lane one pixel of both channels
  constexpr int MAXIT = 16;                                          // (host: S is chosen so that a group needs <= MAXIT)
  float pre[MAXIT][2];
  int poff[4], pix[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int p = min(lane + 64 * q, HW - 1);
    const int py = p / a.W, px = p - py * a.W;
    pix[q] = (lane + 64 * q < HW) ? p : -1;
    poff[q] = ((py + PAD) * PW + (px + PAD)) * xrow;
  }
  auto fetch = [&](int gidx) {
    const int s0 = gidx * a.S;
    const int npl = min(a.S, a.B - s0) * cpairs;
    const float* xg = a.x + (size_t)s0 * a.cin * HW;
    int j = 0, q = 0;
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
        cs_split(v0, h0, m0, l0);
        cs_split(v1, h1, m1, l1);
        unsigned char* dst = Xl + sl * PP * xrow + po + 2 * c;
        typedef __bf16 bf2 __attribute__((ext_vector_type(2)));
        *reinterpret_cast<bf2*>(dst) = (bf2){h0, h1};
        *reinterpret_cast<bf2*>(dst + xplane) = (bf2){m0, m1};
        *reinterpret_cast<bf2*>(dst + 2 * xplane) = (bf2){l0, l1};
      }
      if (++q == ppass) { q = 0; ++j; }
    }
  };

  // ---- this wave's tiles: channel group cg (32 output channels), NR row tiles from rw * NR ----
  const int cgroups = (a.coutp + 31) >> 5, wpc = 8 / cgroups;        // 1 x 8 or 2 x 4 waves
  const int cg = wave / wpc, rw = wave - cg * wpc;
  const int co0 = cg * 32;
  const bool two_co = co0 + 16 < a.coutp;                            // wave-uniform
  const int wbase0 = (co0 + li) * srow, wbase1 = (min(co0 + 16, a.coutp - 16) + li) * srow;

  if ((int)blockIdx.x < ngroups) {
    fetch(blockIdx.x);
    wload(0);
    wstore(0, 0);
  }
  int t = 0;                                                         // slabs walked so far: slab t lives in buffer t & 1
  for (int gidx = blockIdx.x; gidx < ngroups; gidx += gridDim.x) {
    const int s0 = gidx * a.S;
    const int ns = min(a.S, a.B - s0);
    const int R = ns * HW;                                           // live rows of this group
    stage(gidx);
    const bool more = gidx + (int)gridDim.x < ngroups;
    if (more) fetch(gidx + gridDim.x);
    const bool active = rw * NR * 16 < R;                            // wave-uniform
    int xbase[NR];
#pragma unroll
    for (int b = 0; b < NR; ++b) {
      const int r = min((rw * NR + b) * 16 + li, R - 1);
      const int sl = r / HW, p = r - sl * HW;
      const int py = p / a.W, px = p - py * a.W;
      xbase[b] = (sl * PP + py * PW + px) * xrow;
    }
    f32x4 acc[2][NR];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int b = 0; b < NR; ++b) acc[i][b] = (f32x4){0.f, 0.f, 0.f, 0.f};

#pragma unroll 1
    for (int s = 0; s < a.nslab; ++s, ++t) {
      const int nxt = s + 1 < a.nslab ? s + 1 : (more ? 0 : -1);
      if (nxt >= 0) wload(nxt);
      __syncthreads();                                               // slab s (and, at s == 0, the image) is visible; slab s - 1 is done with
      if (active) {
        const int nb = min(a.KS, a.kp - s * a.KS) >> 5;
        const unsigned char* const Wb = Rl + (t & 1) * 3 * splane;
#pragma unroll 1
        for (int blk = 0; blk < nb; ++blk) {
          const int kin = blk * 32 + 8 * lg, kflat = s * a.KS + kin;
          int tap = (int)(((unsigned)kflat * a.mcp) >> 20);
          const int c = kflat - tap * a.cp;
          tap = min(tap, TAPS - 1);                                  // K padding: weights are zero there
          const int dy = tap / KSZ, dx = tap - dy * KSZ;
          const int xoff = (dy * PW + dx) * xrow + 2 * c;
          const int woff = 2 * kin;
          cs_bf16x8 w[2][3];
#pragma unroll
          for (int pl = 0; pl < 3; ++pl) {
            w[0][pl] = *reinterpret_cast<const cs_bf16x8*>(Wb + pl * splane + wbase0 + woff);
            w[1][pl] = *reinterpret_cast<const cs_bf16x8*>(Wb + pl * splane + wbase1 + woff);
          }
#define USF_CS(I, B_, P, Q) acc[I][B_] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w[I][P], xv[Q], acc[I][B_], 0, 0, 0)
#pragma unroll
          for (int b = 0; b < NR; ++b) {
            cs_bf16x8 xv[3];
#pragma unroll
            for (int pl = 0; pl < 3; ++pl) xv[pl] = *reinterpret_cast<const cs_bf16x8*>(Xl + pl * xplane + xbase[b] + xoff);
            USF_CS(0, b, 2, 0); USF_CS(0, b, 1, 1); USF_CS(0, b, 0, 2); USF_CS(0, b, 1, 0); USF_CS(0, b, 0, 1); USF_CS(0, b, 0, 0);
            if (two_co) {
              USF_CS(1, b, 2, 0); USF_CS(1, b, 1, 1); USF_CS(1, b, 0, 2); USF_CS(1, b, 1, 0); USF_CS(1, b, 0, 1); USF_CS(1, b, 0, 0);
            }
          }
#undef USF_CS
        }
      }
      if (nxt >= 0) wstore(nxt, (t + 1) & 1);
    }
    // ---- epilogue: lane (col = li, g = lg) of tile (i, b) holds output channels co0 + 16 i + 4 g + (0..3) of row b * 16 + li
    if (active) {
#pragma unroll
      for (int b = 0; b < NR; ++b) {
        const int r = (rw * NR + b) * 16 + li;
        if (r >= R) continue;
        const int sl = r / HW, p = r - sl * HW;
        float* yb = a.y + ((size_t)(s0 + sl) * a.cout) * HW + p;
        float cx = 0.f;
        unsigned cmask = 0u;
        if constexpr (CTX) {
          const int py = p / a.W;
          cx = a.ctx[(size_t)(s0 + sl) * a.ctx_stride];
          if constexpr (KSZ == 5) cmask = ctx_tapmask5(py, p - py * a.W, a.H, a.W);
          else cmask = ctx_tapmask4(py, p - py * a.W, a.H, a.W);
        }
#pragma unroll
        for (int i = 0; i < 2; ++i) {
          if (i == 1 && !two_co) break;
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const int co = co0 + 16 * i + 4 * lg + j;
            if (co < a.cout) {
              float v = acc[i][b][j] + (a.bias ? a.bias[co] : 0.f);
              if constexpr (CTX && KSZ == 5) v += cx * ctx_tapsum(a.w_ctx + co * TAPS, TAPS, cmask);
              if constexpr (CTX && KSZ == 4) v += cx * ctx_tapsum4(a.w_ctx + co * TAPS, cmask);
              yb[(size_t)co * HW] = act_apply(v, a.out_act, a.out_slope);
            }
          }
        }
      }
    }
    __syncthreads();                                                 // the image is rewritten by the next group
  }
}

static int cs_odd16(int units) { return units | 1; }

// LDS bytes / layout of a launch with S samples per group and slabs of KS
static int64_t conv_stream_lds(int cin, int cout, int H, int W, int ks, int S, int KS, ConvSPlan* p) {
  p->cp = (cin + 7) / 8 * 8;
  p->kp = (ks * ks * p->cp + 31) / 32 * 32;
  p->coutp = (cout + 15) / 16 * 16;
  p->xs16 = cs_odd16(p->cp / 8);
  p->ss16 = cs_odd16(KS / 8);
  const int PP = (H + ks - 1) * (W + ks - 1);
  return 3LL * S * PP * p->xs16 * 16 + 2LL * 3 * p->coutp * p->ss16 * 16;
}

// largest S (<= cap) of a launch with slabs of KS: the LDS (158 KB, as the first kernel), the staging registers and four row
// tiles per wave decide; 0: not one sample fits
static int conv_stream_best_s(int cin, int cout, int H, int W, int ks, int KS, int cap) {
  ConvSPlan p;
  const int coutp = (cout + 15) / 16 * 16, wpc = 8 / ((coutp + 31) / 32);
  for (int S = cap < 8 ? cap : 8; S >= 1; --S)
    if (conv_stream_lds(cin, cout, H, W, ks, S, KS, &p) <= 158 * 1024 && conv_stage_iters(cin, H * W, S) <= 16 &&
        (S * H * W + 15) / 16 <= 4 * wpc) return S;
  return 0;
}

// The streamed kernel's launch for B samples (ks = 5 or 4, sizes inside conv2d_same's rule): slabs of 64 K values unless only
// slabs of 32 bring a second sample into the LDS; S clipped to B; NR = row tiles per wave, rounded up to an instantiation.
int conv_stream_plan(int64_t B, int cin, int cout, int H, int W, int cus, ConvSPlan* p, int ks) {
  const int cap = B < 8 ? (int)B : 8;
  const int s64 = conv_stream_best_s(cin, cout, H, W, ks, 64, 8), s32 = conv_stream_best_s(cin, cout, H, W, ks, 32, 8);
  const int KS = (s64 < 2 && s32 > s64) ? 32 : 64;
  const int best = KS == 64 ? s64 : s32;
  *p = ConvSPlan();
  p->KS = KS; p->depth = 2; p->S_best = best;
  if (best < 1) { p->lds = conv_stream_lds(cin, cout, H, W, ks, 1, KS, p); p->S = 0; return -3; }
  const int S = best < cap ? best : cap;
  p->lds = conv_stream_lds(cin, cout, H, W, ks, S, KS, p);
  p->S = S;
  p->nslab = (p->kp + KS - 1) / KS;
  const int wpc = 8 / ((p->coutp + 31) / 32), per = ((S * H * W + 15) / 16 + wpc - 1) / wpc;
  p->NR = per <= 1 ? 1 : (per == 2 ? 2 : 4);
  if (cus <= 0) cus = device_cu_count();
  p->groups = (B + S - 1) / S;
  p->grid = (unsigned)(p->groups < cus ? p->groups : cus);
  return 0;
}

template <int NR, bool CTX, int KSZ>
static int conv_stream_launch(const ConvSArgs& a5, int pad_before, const ConvSPlan& pl, hipStream_t stream) {
  typename ConvSArgsOf<KSZ>::type a;
  static_cast<ConvSArgs&>(a) = a5;
  if constexpr (KSZ == 4) a.pb = pad_before;
  static bool attr_done[USF_MAX_DEVICES] = {false};
  bool& done = attr_done[current_device_slot()];
  if (!done) {
    if (hipFuncSetAttribute(reinterpret_cast<const void*>(&conv2d_same_stream_kernel<NR, CTX, KSZ>),
                            hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024) != hipSuccess) {
      set_error("usf_conv2d_same_f32: cannot raise the LDS limit");
      return -4;
    }
    done = true;
  }
  hipLaunchKernelGGL((conv2d_same_stream_kernel<NR, CTX, KSZ>), dim3(pl.grid), dim3(512), (size_t)pl.lds, stream, a);
  return check_launch(CTX ? "usf_conv2d_same_ctx_f32" : "usf_conv2d_same_f32");
}

// arguments as conv2d_same has checked them (usf_conv.hip); pl from conv_stream_plan for the same sizes
int conv2d_same_stream(const float* x, float* y, int64_t B, int64_t cin, int64_t cout, int64_t H, int64_t W, const void* wplanes,
                       const float* bias, const float* in_mul, int32_t in_act, float in_slope, int32_t out_act, float out_slope,
                       const float* ctx, int64_t ctx_stride, const float* w_ctx, const ConvSPlan& pl, hipStream_t stream, int ks,
                       int pad_before) {
  ConvSArgs a;
  a.x = x; a.y = y; a.wp = reinterpret_cast<const __bf16*>(wplanes); a.bias = bias; a.in_mul = in_mul;
  a.B = (int)B; a.cin = (int)cin; a.cout = (int)cout; a.H = (int)H; a.W = (int)W;
  a.cp = pl.cp; a.kp = pl.kp; a.coutp = pl.coutp; a.S = pl.S; a.xs16 = pl.xs16; a.ss16 = pl.ss16; a.KS = pl.KS; a.nslab = pl.nslab;
  a.mcp = (1u << 20) / (unsigned)pl.cp + 1u;
  a.in_act = in_act; a.out_act = out_act; a.in_slope = in_slope; a.out_slope = out_slope;
  a.ctx = ctx; a.ctx_stride = (int)ctx_stride; a.w_ctx = w_ctx;
  if ((ks != 4 && ks != 5) || pad_before < 1 || pad_before > 2 || (ks == 5 && pad_before != 2) || pl.kp != (ks * ks * pl.cp + 31) / 32 * 32) {
    set_error("usf_conv2d_same_f32: bad streamed call");
    return -4;
  }
  if (pl.S < 1 || pl.coutp > 64 || pl.KS > 64 || pl.lds > 158 * 1024) { set_error("usf_conv2d_same_f32: bad streamed plan"); return -4; }
#define USF_CS_LAUNCH(KSZ_)                                                              \
  if (ctx) {                                                                             \
    if (pl.NR == 1) return conv_stream_launch<1, true, KSZ_>(a, pad_before, pl, stream);             \
    if (pl.NR == 2) return conv_stream_launch<2, true, KSZ_>(a, pad_before, pl, stream);             \
    return conv_stream_launch<4, true, KSZ_>(a, pad_before, pl, stream);                             \
  }                                                                                      \
  if (pl.NR == 1) return conv_stream_launch<1, false, KSZ_>(a, pad_before, pl, stream);              \
  if (pl.NR == 2) return conv_stream_launch<2, false, KSZ_>(a, pad_before, pl, stream);              \
  return conv_stream_launch<4, false, KSZ_>(a, pad_before, pl, stream)
  if (ks == 5) { USF_CS_LAUNCH(5); }
  USF_CS_LAUNCH(4);
#undef USF_CS_LAUNCH
}

}  // namespace usf
