// Row-banded "same" convolution for feature maps the resident-sample kernel of usf_conv.hip cannot hold:
// 257 .. 4096 pixels (MNIST 28 x 28, CIFAR 32 x 32 without space-to-depth), kernel 1 x 1 or 3 x 3, stride 1, inference only.
//
//   y[b, co, p] = out_act( bias[co] + [ctx term] + sum_{tap, ci} W[co, ci, tap] * a[b, ci, p + tap] ),   a = in_act(x) * in_mul
//
// The arithmetic, the weight planes, the LDS layouts and the epilogue are conv2d_same_bf16x3_kernel's (usf_conv.hip: bf16x3
// split in the staging pass, six v_mfma_f32_16x16x32_bf16 per product, patch shapes from conv_patch_shape).  The difference is
// the GROUP a persistent 512-thread block works on: a band of RB consecutive output rows of ONE sample,
//   * LDS image: (RB + ks - 1) x (W + ks - 1) positions x Cp channels x 3 planes beside the resident weight planes;
//   * staged input: the contiguous pixel range of the rows r0 - pad .. r0 + RB - 1 + pad, clipped to the image, of every channel
//     plane -- coalesced 64-pixel passes, at most MAXIT = 16 register-staged iterations per thread (the plan bounds RB by it);
//   * group g = (sample g / nbands, band g % nbands): neighbouring blocks share their halo rows in L2.
// What the resident-sample kernel does not have to care about:
//   * halo rows: the top / bottom rows of the image hold data for an interior band and must read as zero for a sample's first /
//     last band (and below a ragged last band).  A block walks from one kind of band to the other, so every group whose halo
//     falls outside the sample clears those image rows itself; the left / right border columns and the padding channels are
//     never written after the one clear at the start of the block;
//   * pixel indices: in_mul, the context's edge / corner class and the output address use the ABSOLUTE row r0 + (row in band);
//   * an output element's sum order (k-blocks in order, the six products in the first kernel's order) depends on neither RB, the
//     band, the patch shape nor the group's place in the grid: the same bits for every banding.
#include "usf_common.h"
#include "usf_conv_plan.h"
#include <type_traits>

namespace usf {

typedef __bf16 cb_bf16x8 __attribute__((ext_vector_type(8)));

struct ConvBArgs {
  const float* x; float* y;
  const __bf16* wp;            // [3][coutp][kp]
  const float* bias;           // [cout] or null
  const float* in_mul;         // [cin * hw] or null
  int cin, cout, H, W, ks;
  int cp, kp, coutp;           // padded channel count, padded K, padded Cout (multiple of 16)
  int RB, nbands;              // output rows per band, bands per sample
  int ngroups;                 // B * nbands
  int npass;                   // 64-pixel passes over the staged rows of a full band
  unsigned mW;                 // floor(2^32 / W) + 1: n / W = umulhi(n, mW) for n < 2^26 (W >= 2; W == 1 divides by nothing)
  int xs16, ws16;              // LDS row strides in 16-byte units (odd)
  int in_act, out_act; float in_slope, out_slope;
  const float* ctx; int ctx_stride;   // context channel (CTX instantiation only): ctx[b * ctx_stride]
  const float* w_ctx;          // [cout][ks * ks] weights of the context channel
};

__device__ __forceinline__ void cb_split(float x, __bf16& h, __bf16& m, __bf16& l) {
  h = (__bf16)x;
  const float r = x - (float)h;
  m = (__bf16)r;
  l = (__bf16)(r - (float)m);
}

// CTX: the context channel's rank-1 term joins the bias in the epilogue (as usf_conv2d_same_ctx_f32); false: the plain form
template <bool CTX>
__global__ __launch_bounds__(512, 2) void conv2d_same_band_kernel(const ConvBArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int li = lane & 15, lg = lane >> 4;
  const int HW = a.H * a.W;
  const int pad = a.ks >> 1;
  const int PW = a.W + 2 * pad, PP = (a.RB + 2 * pad) * PW;          // the band's padded image
  const int taps = a.ks * a.ks;
  const int wrow = a.ws16 * 16, xrow = a.xs16 * 16;                  // bytes per LDS row
  const int wplane = a.coutp * wrow, xplane = PP * xrow;             // bytes per plane
  unsigned char* const Wl = smem;
  unsigned char* const Xl = smem + 3 * wplane;
  const f32x4 z4 = {0.f, 0.f, 0.f, 0.f};

  // ---- once per block: weights into LDS, the image zeroed (border columns and padding channels stay zero) ----
  {
    const int units = a.kp / 8;                                      // 16-byte units per weight row
    for (int i = tid; i < 3 * a.coutp * units; i += 512) {
      const int pl = i / (a.coutp * units), rem = i % (a.coutp * units);
      const int r = rem / units, u = rem % units;
      *reinterpret_cast<cb_bf16x8*>(Wl + pl * wplane + r * wrow + u * 16) =
          *reinterpret_cast<const cb_bf16x8*>(a.wp + ((size_t)(pl * a.coutp + r) * a.kp + 8 * u));
    }
    for (int i = tid; i < 3 * xplane / 16; i += 512) *reinterpret_cast<f32x4*>(Xl + i * 16) = z4;
  }
  __syncthreads();

  const int nblk = a.kp / 32;
  auto div_w = [&](int n) { return a.W == 1 ? n : (int)__umulhi((unsigned)n, a.mW); };
  // Staging: a wave takes channel-pair planes, a lane one pixel of both channels -- two coalesced loads, two splits, three
  // 4-byte LDS stores.  Iteration `it` is (plane round j, pixel pass q), both wave-uniform counters: the pixel is
  // first staged pixel + lane + 64 q, its row and column come from one multiply -- no table indexed at run time.  The loads of
  // the block's next group are issued before the MFMA phase of this one and consumed after it.
  constexpr int MAXIT = 16;                                          // (host: RB is chosen so that a band needs <= MAXIT)
  float pre[MAXIT][2];
  auto fetch = [&](int gidx) {
    const int smp = gidx / a.nbands, r0 = (gidx - smp * a.nbands) * a.RB;
    const int rb = min(a.RB, a.H - r0);
    const int plo = max(r0 - pad, 0) * a.W, phi = min(r0 + rb + pad, a.H) * a.W;   // staged pixels of every channel plane
    const float* xg = a.x + (size_t)smp * a.cin * HW;
    int j = 0, q = 0;
#pragma unroll
    for (int it = 0; it < MAXIT; ++it) {
      const int c = 2 * (wave + 8 * j);
      const int p = plo + lane + 64 * q;
      pre[it][0] = pre[it][1] = 0.f;
      if (c < a.cin && p < phi) {
        const float* x0 = xg + (size_t)c * HW + p;
        pre[it][0] = x0[0];
        if (c + 1 < a.cin) pre[it][1] = x0[HW];
      }
      if (++q == a.npass) { q = 0; ++j; }
    }
  };
  auto stage = [&](int gidx) {
    const int smp = gidx / a.nbands, r0 = (gidx - smp * a.nbands) * a.RB;
    const int rb = min(a.RB, a.H - r0);
    const int plo = max(r0 - pad, 0) * a.W, phi = min(r0 + rb + pad, a.H) * a.W;
    if (pad > 0) {
      // halo rows outside the sample: image rows [0, pad) of a first band, [rb + pad, rb + 2 pad) of a last band -- whole image
      // rows, all three planes (an interior band staged real rows there; rows below a ragged band's halo are never read)
      const int units = pad * PW * a.xs16;
      if (r0 - pad < 0)
        for (int i = tid; i < 3 * units; i += 512) {
          const int pl = i / units, u = i - pl * units;
          *reinterpret_cast<f32x4*>(Xl + pl * xplane + u * 16) = z4;
        }
      if (r0 + rb + pad > a.H)
        for (int i = tid; i < 3 * units; i += 512) {
          const int pl = i / units, u = i - pl * units;
          *reinterpret_cast<f32x4*>(Xl + pl * xplane + (rb + pad) * PW * xrow + u * 16) = z4;
        }
    }
    int j = 0, q = 0;
#pragma unroll
    for (int it = 0; it < MAXIT; ++it) {
      const int c = 2 * (wave + 8 * j);
      const int p = plo + lane + 64 * q;
      if (c < a.cin && p < phi) {
        const int py = div_w(p), px = p - py * a.W;                  // absolute row / column
        float v0 = act_apply(pre[it][0], a.in_act, a.in_slope), v1 = act_apply(pre[it][1], a.in_act, a.in_slope);
        if (a.in_mul) {
          v0 *= a.in_mul[c * HW + p];
          if (c + 1 < a.cin) v1 *= a.in_mul[(c + 1) * HW + p];
        }
        __bf16 h0, m0, l0, h1, m1, l1;
        cb_split(v0, h0, m0, l0);
        cb_split(v1, h1, m1, l1);
        unsigned char* dst = Xl + ((py - r0 + pad) * PW + (px + pad)) * xrow + 2 * c;
        typedef __bf16 bf2 __attribute__((ext_vector_type(2)));
        *reinterpret_cast<bf2*>(dst) = (bf2){h0, h1};
        *reinterpret_cast<bf2*>(dst + xplane) = (bf2){m0, m1};
        *reinterpret_cast<bf2*>(dst + 2 * xplane) = (bf2){l0, l1};
      }
      if (++q == a.npass) { q = 0; ++j; }
    }
  };
  if ((int)blockIdx.x < a.ngroups) fetch(blockIdx.x);
  for (int gidx = blockIdx.x; gidx < a.ngroups; gidx += gridDim.x) {
    const int smp = gidx / a.nbands, r0 = (gidx - smp * a.nbands) * a.RB;
    const int R = min(a.RB, a.H - r0) * a.W;                         // live GEMM rows of this band: its output pixels
    stage(gidx);
    __syncthreads();
    if (gidx + (int)gridDim.x < a.ngroups) fetch(gidx + gridDim.x);
    // ---- implicit GEMM: (co) x (pixels of the band) patches dealt over the waves, as in conv2d_same_bf16x3_kernel ----
    auto patches = [&](auto pc_, auto pr_) {
      constexpr int PC = decltype(pc_)::value, PR = decltype(pr_)::value;      // 16-row tiles per patch in co / rows
      const int ctn = (a.coutp / 16 + PC - 1) / PC, rtn = (R + 16 * PR - 1) / (16 * PR);
      for (int t = wave; t < ctn * rtn; t += 8) {
        const int ct = t / rtn, rt = t - ct * rtn;
        // this lane's row positions (B operand columns): row r -> (row in band, column) -> top-left of its window
        int xbase[PR];
#pragma unroll
        for (int b = 0; b < PR; ++b) {
          const int r = min(rt * 16 * PR + b * 16 + li, R - 1);
          const int ly = div_w(r), lx = r - ly * a.W;
          xbase[b] = (ly * PW + lx) * xrow;
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
          for (int b = 0; b < PR; ++b) acc[i][b] = z4;
        cb_bf16x8 wf[2][PC][3], xf[2][PR][3];                            // [buffer][tile][plane]: block k + 1 is read under block k
        auto read_blk = [&](int blk, cb_bf16x8 (&w)[PC][3], cb_bf16x8 (&xv)[PR][3]) {
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
            for (int i = 0; i < PC; ++i) w[i][pl] = *reinterpret_cast<const cb_bf16x8*>(Wl + pl * wplane + wbase[i] + woff);
#pragma unroll
            for (int b = 0; b < PR; ++b) xv[b][pl] = *reinterpret_cast<const cb_bf16x8*>(Xl + pl * xplane + xbase[b] + xoff);
          }
        };
        auto mm_blk = [&](const cb_bf16x8 (&w)[PC][3], const cb_bf16x8 (&xv)[PR][3]) {
#define USF_CB(I, B_, P, Q) acc[I][B_] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(w[I][P], xv[B_][Q], acc[I][B_], 0, 0, 0)
#pragma unroll
          for (int b = 0; b < PR; ++b) {
            USF_CB(0, b, 2, 0); USF_CB(0, b, 1, 1); USF_CB(0, b, 0, 2); USF_CB(0, b, 1, 0); USF_CB(0, b, 0, 1); USF_CB(0, b, 0, 0);
            if (PC == 2 && two_co) {
              USF_CB(PC - 1, b, 2, 0); USF_CB(PC - 1, b, 1, 1); USF_CB(PC - 1, b, 0, 2); USF_CB(PC - 1, b, 1, 0); USF_CB(PC - 1, b, 0, 1);
              USF_CB(PC - 1, b, 0, 0);
            }
          }
#undef USF_CB
        };
        read_blk(0, wf[0], xf[0]);
        int blk = 0;
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
          float* yb = a.y + ((size_t)smp * a.cout) * HW + (r0 * a.W + r);   // the pixel's absolute index
          float cx = 0.f;
          unsigned cmask = 0u;
          if constexpr (CTX) {
            const int ly = div_w(r);
            cx = a.ctx[(size_t)smp * a.ctx_stride];
            cmask = ctx_tapmask(r0 + ly, r - ly * a.W, a.H, a.W, a.ks);
          }
#pragma unroll
          for (int i = 0; i < PC; ++i) {
            if (i == 1 && !two_co) break;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
              const int co = co0 + 16 * i + 4 * lg + j;
              if (co < a.cout) {
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
    const int shape = conv_patch_shape(a.coutp, R, 0);
    if (shape == 0x22) patches(I2(), I2());
    else if (shape == 0x12) patches(I1(), I2());
    else patches(I1(), I1());
    __syncthreads();                                                 // the image is rewritten by the next group
  }
}

// ---- the plan (usf_conv_plan.h): host only ------------------------------------------------------------------------------------
static int cb_odd16(int units) { return units | 1; }

// The band of a shape: the most output rows whose image fits 158 KiB of LDS beside the weight planes and whose staged rows fit
// the MAXIT register-staged iterations, at most H.  Not served (1): sizes outside 1..64 channels, W <= 64, H W <= 4096, ks 1 / 3;
// not even one row fits; or, at ks = 3, a best band below 4 rows of a map that has 4 (the halo would make the staged bytes more
// than 1.5 x the image).  band_rows > 0 caps the band (a measurement and test aid); cus <= 0 asks the device.
int conv_band_plan(int64_t B, int64_t cin_, int64_t cout_, int64_t H_, int64_t W_, int64_t ks_, int band_rows, int cus, ConvBPlan* p) {
  *p = ConvBPlan();
  if (cin_ <= 0 || cout_ <= 0 || H_ <= 0 || W_ <= 0 || cin_ > 64 || cout_ > 64 || W_ > 64 || H_ * W_ > 4096 || (ks_ != 1 && ks_ != 3))
    return 1;
  const int cin = (int)cin_, cout = (int)cout_, H = (int)H_, W = (int)W_, ks = (int)ks_;
  const int cp = (cin + 7) / 8 * 8, kp = (ks * ks * cp + 31) / 32 * 32, coutp = (cout + 15) / 16 * 16;
  p->cp = cp; p->kp = kp; p->coutp = coutp;
  p->xs16 = cb_odd16(cp / 8); p->ws16 = cb_odd16(kp / 8);
  p->wbytes = 3LL * coutp * p->ws16 * 16;
  const int PW = W + ks - 1;
  auto lds_of = [&](int rb) { return p->wbytes + 3LL * (rb + ks - 1) * PW * p->xs16 * 16; };
  int best = 0;
  for (int rb = H; rb >= 1; --rb)
    if (lds_of(rb) <= 158 * 1024 && conv_band_stage_iters(cin, W, rb + ks - 1) <= 16) { best = rb; break; }
  p->RB_best = best;
  if (best < 1 || (ks == 3 && best < 4 && best < H)) return 1;
  const int RB = band_rows > 0 && band_rows < best ? band_rows : best;
  p->RB = RB;
  p->nbands = (H + RB - 1) / RB;
  p->last_rows = H - (p->nbands - 1) * RB;
  p->iters = conv_band_stage_iters(cin, W, RB + ks - 1);
  p->npass = ((RB + ks - 1) * W + 63) / 64;
  p->lds = lds_of(RB);
  p->groups = B > 0 ? B * p->nbands : 0;
  if (p->groups > 0x7fffffff) return 1;
  if (cus <= 0) cus = device_cu_count();
  p->grid = (unsigned)(p->groups < cus ? p->groups : cus);
  return 0;
}

int conv2d_same_band_fits(int64_t cin, int64_t cout, int64_t H, int64_t W, int64_t ks) {
  ConvBPlan p;
  return conv_band_plan(1, cin, cout, H, W, ks, 0, 1, &p) == 0 ? p.RB_best : 0;
}

int conv2d_same_band_variant(const usf_conv_band_query* q, usf_conv_band_info* o) {
  if (!q || !o) { set_error("usf_conv2d_same_band_variant: null pointer"); return -1; }
  *o = usf_conv_band_info();
  if (q->B <= 0 || q->B > 0x7fffffff || q->band_rows < 0) return 0;
  ConvBPlan p;
  const int rc = conv_band_plan(q->B, q->cin, q->cout, q->H, q->W, q->ks, q->band_rows, q->cus > 0 ? q->cus : device_cu_count(), &p);
  o->best_rows = p.RB_best; o->weight_bytes = p.wbytes;
  if (rc != 0) return 0;
  o->served = 1; o->band_rows = p.RB; o->bands = p.nbands; o->last_rows = p.last_rows;
  o->groups = p.groups; o->grid = p.grid; o->lds_bytes = p.lds;
  o->stage_iters = p.iters; o->CTX = q->ctx != 0;
  const int full = conv_patch_shape(p.coutp, p.RB * (int)q->W, 0), last = conv_patch_shape(p.coutp, p.last_rows * (int)q->W, 0);
  o->PC_full = full >> 4; o->PR_full = full & 15; o->PC_last = last >> 4; o->PR_last = last & 15;
  return 0;
}

int conv2d_same_band(const float* x, float* y, int64_t B, int64_t cin, int64_t cout, int64_t H, int64_t W, int64_t ks,
                     const void* wplanes, const float* bias, const float* in_mul, int32_t in_act, float in_slope, int32_t out_act,
                     float out_slope, const float* ctx, int64_t ctx_stride, const float* w_ctx, int64_t band_rows, hipStream_t stream) {
  if (B < 0 || cin <= 0 || cout <= 0 || H <= 0 || W <= 0 || ks <= 0 || B > 0x7fffffff || band_rows < 0 || band_rows > 0x7fffffff) {
    set_error("usf_conv2d_same_band_f32: bad sizes");
    return -2;
  }
  for (int32_t act : {in_act, out_act})
    if (act != USF_ACT_NONE && act != USF_ACT_LEAKY_RELU) { set_error("usf_conv2d_same_band_f32: bad act"); return -2; }
  if (ctx && (!w_ctx || (ctx_stride != 0 && ctx_stride != 1))) {
    set_error("usf_conv2d_same_band_f32: the context channel wants w_ctx and ctx_stride 0 or 1");
    return -2;
  }
  if (B == 0) return 0;
  ConvBPlan pl;
  if (conv_band_plan(B, cin, cout, H, W, ks, (int)band_rows, 1, &pl) != 0) return 1;   // (a valid shape this kernel does not serve)
  if (!x || !y || !wplanes) { set_error("usf_conv2d_same_band_f32: null pointer"); return -1; }
  if (x == y) { set_error("usf_conv2d_same_band_f32: in-place operation is not supported"); return -2; }
  if (!aligned16(wplanes)) { set_error("usf_conv2d_same_band_f32: weight planes must be 16-byte aligned"); return -2; }
  conv_band_plan(B, cin, cout, H, W, ks, (int)band_rows, 0, &pl);                        // ... now for this device's compute units
  ConvBArgs a;
  a.x = x; a.y = y; a.wp = reinterpret_cast<const __bf16*>(wplanes); a.bias = bias; a.in_mul = in_mul;
  a.cin = (int)cin; a.cout = (int)cout; a.H = (int)H; a.W = (int)W; a.ks = (int)ks;
  a.cp = pl.cp; a.kp = pl.kp; a.coutp = pl.coutp;
  a.RB = pl.RB; a.nbands = pl.nbands; a.ngroups = (int)pl.groups; a.npass = pl.npass;
  a.mW = W > 1 ? (unsigned)((1ULL << 32) / (uint64_t)W) + 1u : 0u;
  a.xs16 = pl.xs16; a.ws16 = pl.ws16;
  a.in_act = in_act; a.out_act = out_act; a.in_slope = in_slope; a.out_slope = out_slope;
  a.ctx = ctx; a.ctx_stride = (int)ctx_stride; a.w_ctx = w_ctx;
  static bool attr_done_dev[2][USF_MAX_DEVICES] = {{false}};   // (the attribute belongs to the device and the instantiation)
  bool& attr_done = attr_done_dev[ctx ? 1 : 0][current_device_slot()];
  if (!attr_done) {
    const void* kfn = ctx ? reinterpret_cast<const void*>(&conv2d_same_band_kernel<true>)
                          : reinterpret_cast<const void*>(&conv2d_same_band_kernel<false>);
    if (hipFuncSetAttribute(kfn, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024) != hipSuccess) {
      set_error("usf_conv2d_same_band_f32: cannot raise the LDS limit");
      return -4;
    }
    attr_done = true;
  }
  if (ctx) hipLaunchKernelGGL(conv2d_same_band_kernel<true>, dim3(pl.grid), dim3(512), (size_t)pl.lds, stream, a);
  else hipLaunchKernelGGL(conv2d_same_band_kernel<false>, dim3(pl.grid), dim3(512), (size_t)pl.lds, stream, a);
  return check_launch("usf_conv2d_same_band_f32");
}

}  // namespace usf
