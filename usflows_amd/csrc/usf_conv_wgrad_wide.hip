// Weight / bias gradient of a stride-1 "same" convolution (kernel 1 or 3) for feature maps of up to 256 pixels and ANY channel
// counts up to 64 (usf_conv_wgrad_wide_f32): the contract of usf_conv_wgrad_f32 (usf_image_grad.hip)
//     dW[co, ci, tap] = sum_{b, p} dy[b, co, p] * xin[b, ci, p + tap],   db[co] = sum_{b, p} dy[b, co, p],
//     xin = in_act(x - pre_sub[ci]) * in_mul, zeros outside the image,
// exact fp32 on v_mfma_f32_16x16x4_f32 (A = dy[16 co][4 positions], B = x[16 ci][4 shifted positions] -> D[co][ci]).
//
// usf_conv_wgrad_f32 keeps a whole sample per WAVE in LDS, which ends at 64 pixels.  Here one 256-thread BLOCK owns one sample
// at a time: it stages the sample into LDS as x [cinp][CSx] and dy [coutp][CSy] (cinp / coutp = the channel counts rounded up
// to 16; the channels past the real ones stay zero for the whole launch).  Kernel 3 uses the row stride S = W + 1 with a zero
// row above and below the x image, so a tap is a constant offset and a column wrap-around lands on a real zero; dy has zeros in
// its pad column, so the padded positions add exact zeros.  The channel strides are 2 * odd: the 32 lanes of a ds_read_b32
// group (16 channels x 2 positions) hit 32 banks.
// db rides on the same instruction: every cout tile has one more tile whose B operand is a row of ones in LDS, so all 16
// columns of its result hold sum dy[co] -- the same k-ordered fma chain, no vector-ALU work beside the MFMAs.
// The accumulator tiles -- per cout tile CIT * T weight tiles (cin tile, tap) and the bias tile, at most 4 * (4 * 9 + 1) = 148
// -- are dealt over the waves: tile g belongs to wave group g % TG and is that group's tile g / TG (NT = ceil(tiles / TG) tiles
// of 4 registers per wave, NT <= 37).  With two tiles (16 -> 16 channels at kernel 1) the two waves left over split the sample's
// position chunks instead (PS = 4 / TG parts).  One barrier pair per sample; the accumulators live across the block's samples
// and leave once, to a partial slot of the block's own (slot = block * PS + part), and a fixed-order sum over the slots
// follows: same bits on every run, no atomics.
#include "usf_common.h"

namespace usf {
namespace {

struct WwArgs {
  const float* x;
  const float* dy;
  float* part;             // [slots][nacc]
  const float* in_mul;     // [cin * HW] or NULL
  const float* pre_sub;    // [cin] or NULL
  int B, cin, cout, HW, W, S, CSx, CSy, q0, nch, nex, ney, nacc;
  int CIT, T, ntiles, TG, PS, lds_floats;
  unsigned m_hw, m_w;      // ceil(2^32 / HW), ceil(2^32 / W); 0: the divisor is 1
  float slope_eff;         // leaky slope of the input nonlinearity; 1 = none
};

__device__ __forceinline__ int ww_div(int e, unsigned magic) { return magic ? (int)__umulhi((unsigned)e, magic) : e; }

template <int NT>
__global__ __launch_bounds__(256) void conv_wgrad_wide_kernel(const WwArgs a) {
  extern __shared__ __attribute__((aligned(16))) float ww_lds[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int cinp = a.CIT * 16;
  float* xl = ww_lds;                                           // [cinp][CSx], then the row of ones
  float* dl = ww_lds + (cinp + 1) * a.CSx;                      // [coutp][CSy]
  for (int i = tid; i < a.lds_floats; i += 256) ww_lds[i] = 0.f;   // padding rows, columns and channels: zero for the whole launch
  __syncthreads();
  for (int i = tid; i < a.CSx; i += 256) xl[cinp * a.CSx + i] = 1.f;

  // this wave's tiles: g = tg + TG * k (a k past the last tile repeats the wave's first one; its sums are never written).
  // The fragment addresses are per-lane values on purpose (tid >> 6, not the wave-uniform copy): 2 * NT of them stay in
  // vector registers instead of spilling out of the scalar file.
  const int tg = wave % a.TG, ps = wave / a.TG;
  const int per_cot = a.CIT * a.T + 1;
  int pa[NT], pb[NT];
  {
    const int tgv = (tid >> 6) % a.TG;
    const int la = (lane & 15) * a.CSy + (lane >> 4);
    const int lb = (lane & 15) * a.CSx + (lane >> 4);
#pragma unroll
    for (int k = 0; k < NT; ++k) {
      const int g = tgv + a.TG * k;
      const int gg = g < a.ntiles ? g : tgv;
      const int cot = gg / per_cot, rem = gg - cot * per_cot;
      pa[k] = cot * 16 * a.CSy + la;
      if (rem == per_cot - 1) {
        pb[k] = cinp * a.CSx + (lane >> 4);                     // the bias tile: B = ones, D[co][*] = sum dy[co]
      } else {
        const int cit = rem / a.T, t = rem - cit * a.T;
        const int toff = (a.T == 9) ? (t / 3 - 1) * a.S + (t % 3 - 1) : 0;
        pb[k] = cit * 16 * a.CSx + a.q0 + toff + lb;
      }
    }
  }
  f32x4 acc[NT];
#pragma unroll
  for (int k = 0; k < NT; ++k) acc[k] = f32x4{0.f, 0.f, 0.f, 0.f};
  const int c0 = ps * a.nch / a.PS, c1 = (ps + 1) * a.nch / a.PS;   // this wave's range of the position chunks
  const int pad = a.S - a.W;
  const bool has_ps = a.pre_sub != nullptr, has_mul = a.in_mul != nullptr;

  for (int s = blockIdx.x; s < a.B; s += gridDim.x) {
    const float* xs = a.x + (int64_t)s * a.nex;
    const float* ys = a.dy + (int64_t)s * a.ney;
    __syncthreads();                                            // the fills / the previous sample's fragment reads are done
    for (int e0 = tid; e0 < a.nex; e0 += 1024) {
      float v[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int e = e0 + 256 * u;
        v[u] = e < a.nex ? xs[e] : 0.f;
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int e = e0 + 256 * u;
        if (e < a.nex) {
          const int c = ww_div(e, a.m_hw), p = e - c * a.HW, r = ww_div(p, a.m_w);
          float val = v[u];
          if (has_ps) val -= a.pre_sub[c];
          val = val > 0.f ? val : val * a.slope_eff;
          if (has_mul) val *= a.in_mul[e];
          xl[c * a.CSx + a.q0 + p + r * pad] = val;
        }
      }
    }
    for (int e0 = tid; e0 < a.ney; e0 += 1024) {
      float v[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int e = e0 + 256 * u;
        v[u] = e < a.ney ? ys[e] : 0.f;
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int e = e0 + 256 * u;
        if (e < a.ney) {
          const int c = ww_div(e, a.m_hw), p = e - c * a.HW, r = ww_div(p, a.m_w);
          dl[c * a.CSy + p + r * pad] = v[u];
        }
      }
    }
    __syncthreads();
    if (tg < a.ntiles) {
      for (int ch = c0; ch < c1; ++ch) {
#pragma unroll
        for (int k = 0; k < NT; ++k)
          acc[k] = __builtin_amdgcn_mfma_f32_16x16x4f32(dl[pa[k] + 4 * ch], xl[pb[k] + 4 * ch], acc[k], 0, 0, 0);
      }
    }
  }

  // this wave's partial sums: tile g at [g * 256 + register * 64 + lane]
  float* pw = a.part + ((int64_t)blockIdx.x * a.PS + ps) * a.nacc;
#pragma unroll
  for (int k = 0; k < NT; ++k) {
    const int g = tg + a.TG * k;
    if (g < a.ntiles) {
#pragma unroll
      for (int r = 0; r < 4; ++r) pw[g * 256 + r * 64 + lane] = acc[k][r];
    }
  }
}

// out[j] = the sum over the partial slots [by * per, min((by + 1) * per, nparts)) in a fixed order: four interleaved chains,
// then ((0 + 1) + 2) + 3 -- the order of usf_conv_wgrad_f32's rounds.  mode 0: row `by` of out.  mode 1: the slot layout above
// -> dW [cout][cin][T] and db [cout] (the padded channels are dropped).
__global__ __launch_bounds__(256) void conv_wgrad_wide_sum_kernel(const float* __restrict__ part, int nparts, int per, int n,
                                                                  float* __restrict__ out, float* __restrict__ out2, int mode, int cin,
                                                                  int cout, int CIT, int T) {
  __shared__ float red[4][64];
  const int jj = threadIdx.x & 63, g = threadIdx.x >> 6;
  const int j = blockIdx.x * 64 + jj, by = blockIdx.y;
  const int p0 = by * per, p1 = (p0 + per < nparts) ? p0 + per : nparts;
  float s = 0.f;
  if (j < n)
    for (int p = p0 + g; p < p1; p += 4) s += part[(int64_t)p * n + j];
  red[g][jj] = s;
  __syncthreads();
  if (g != 0 || j >= n) return;
  const float total = ((red[0][jj] + red[1][jj]) + red[2][jj]) + red[3][jj];
  if (mode == 0) {
    out[(int64_t)by * n + j] = total;
    return;
  }
  // (T: the taps; a cout tile owns CIT * T weight tiles and behind them its bias tile, whose 16 columns all hold db)
  const int tile = j >> 8, r = (j >> 6) & 3, ln = j & 63;
  const int per_cot = CIT * T + 1;
  const int cot = tile / per_cot, rem = tile - cot * per_cot;
  const int co = cot * 16 + 4 * (ln >> 4) + r;
  if (co >= cout) return;
  if (rem == per_cot - 1) {
    if (out2 && (ln & 15) == 0) out2[co] = total;
    return;
  }
  const int cit = rem / T, t = rem - cit * T;
  const int ci = cit * 16 + (ln & 15);
  if (ci < cin) out[((int64_t)co * cin + ci) * T + t] = total;
}

constexpr int kWideReduceRows = 64;     // scratch rows of the two-round sum (workspace: that many * nacc floats behind the slots)
constexpr int kWideLdsMax = 160 * 1024;

// rounds of the sum of `nparts` slots: 1 up to 64 slots; else 2: a first round of `used` rows (<= 64) of `per` slots each
int wide_rounds(int nparts, int& per, int& used) {
  per = nparts;
  used = 1;
  if (nparts <= 64) return 1;
  const int rows = nparts / 16 < kWideReduceRows ? (nparts + 15) / 16 : kWideReduceRows;
  per = (nparts + rows - 1) / rows;
  used = (nparts + per - 1) / per;
  return 2;
}

unsigned wide_magic(int d) { return d < 2 ? 0u : (unsigned)((0x100000000ULL + (unsigned)d - 1) / (unsigned)d); }

int two_odd_at_least(int need) {
  int h = (need + 1) / 2;
  if (!(h & 1)) ++h;
  return 2 * h;
}

#define USF_WW_INSTANCES(X) X(1) X(2) X(3) X(4) X(5) X(7) X(8) X(10) X(14) X(15) X(19) X(21) X(28) X(37)

struct WwPlan {
  int CIT, COT, T, S, q0, nch, CSx, CSy, ntiles, TG, PS, NT, nacc, lds_floats, lds_bytes, blocks, slots, per_cu, cus;
};

// cus / blocks_per_cu <= 0: the device's compute units (256 when there is no device) / the residency the LDS image allows
bool wide_plan(int64_t B, int64_t cin, int64_t cout, int64_t H, int64_t W, int64_t ks, int cus, int blocks_per_cu, WwPlan& pl) {
  if (B <= 0 || B > 0x7fffffff || cin <= 0 || cout <= 0 || cin > 64 || cout > 64 || H <= 0 || W <= 0 || H > 256 || W > 256 ||
      H * W > 256 || (ks != 1 && ks != 3))
    return false;
  pl.CIT = (int)(cin + 15) / 16;
  pl.COT = (int)(cout + 15) / 16;
  pl.T = (int)(ks * ks);
  const int HW = (int)(H * W);
  if (ks == 3) {
    pl.S = (int)W + 1;
    pl.q0 = pl.S + 1;
    pl.nch = (int)((H - 1) * pl.S + W + 3) / 4;                  // padded positions from the first to the last pixel, in fours
    pl.CSy = two_odd_at_least(4 * pl.nch);
    pl.CSx = two_odd_at_least(pl.q0 + 4 * pl.nch + pl.S + 1);     // last position a fragment read touches + 1
  } else {
    pl.S = (int)W;
    pl.q0 = 0;
    pl.nch = (HW + 3) / 4;
    pl.CSx = pl.CSy = two_odd_at_least(4 * pl.nch);
  }
  pl.lds_floats = (pl.CIT * 16 + 1) * pl.CSx + pl.COT * 16 * pl.CSy;     // (+ the row of ones: the bias tile's B operand)
  pl.lds_bytes = pl.lds_floats * 4;
  if (pl.lds_bytes > kWideLdsMax) return false;                   // (tall, narrow maps of many channels: the pad column doubles them)
  pl.ntiles = pl.COT * (pl.CIT * pl.T + 1);                      // (+ one bias tile per cout tile)
  pl.TG = pl.ntiles >= 3 ? 4 : pl.ntiles;
  pl.PS = 4 / pl.TG;
  pl.NT = (pl.ntiles + pl.TG - 1) / pl.TG;
  pl.nacc = pl.ntiles * 256;
  int per_cu = blocks_per_cu > 0 ? blocks_per_cu : kWideLdsMax / pl.lds_bytes;
  pl.per_cu = per_cu;
  if (per_cu > 2) per_cu = 2;                                     // (more partial slots than that buy nothing)
  pl.cus = cus > 0 ? cus : device_cu_count();
  int64_t blocks = B;
  if (blocks > (int64_t)pl.cus * per_cu) blocks = (int64_t)pl.cus * per_cu;
  pl.blocks = (int)blocks;
  pl.slots = pl.blocks * pl.PS;
  return true;
}

}  // namespace

int conv_wgrad_wide_variant(const usf_conv_wgrad_query* q, usf_conv_wgrad_wide_info* o) {
  if (!q || !o) { set_error("usf_conv_wgrad_wide_variant: null pointer"); return -1; }
  *o = usf_conv_wgrad_wide_info();
  WwPlan pl;
  if (!wide_plan(q->B, q->cin, q->cout, q->H, q->W, q->ks, q->cus, q->blocks_per_cu, pl)) return 0;
  o->served = 1;
  o->CIT = pl.CIT; o->COT = pl.COT; o->T = pl.T; o->tiles = pl.ntiles; o->tiles_per_wave = pl.NT; o->wave_groups = pl.TG;
  o->position_parts = pl.PS; o->blocks = pl.blocks; o->lds_bytes = pl.lds_bytes; o->S = pl.S; o->q0 = pl.q0; o->CSx = pl.CSx;
  o->CSy = pl.CSy; o->nch = pl.nch; o->nacc = pl.nacc; o->slots = pl.slots;
  int per, used;
  o->rounds = wide_rounds(pl.slots, per, used);
  o->per = per;
  o->rows_used = used;
  o->max_samples_per_block = (int32_t)((q->B + pl.blocks - 1) / pl.blocks);
  o->blocks_per_cu = pl.per_cu;
  o->cus = pl.cus;
  return 0;
}

int64_t conv_wgrad_wide_workspace(int64_t B, int64_t cin, int64_t cout, int64_t H, int64_t W, int64_t ks) {
  WwPlan pl;
  if (!wide_plan(B, cin, cout, H, W, ks, 0, 0, pl)) return 0;
  return ((int64_t)pl.slots + kWideReduceRows) * pl.nacc;
}

int conv_wgrad_wide(const float* x, const float* dy, int64_t B, int64_t cin, int64_t cout, int64_t H, int64_t W, int64_t ks,
                    const float* in_mul, const float* pre_sub, int32_t in_act, float in_slope, float* dW, float* db,
                    float* workspace, int64_t workspace_floats, hipStream_t stream) {
  WwPlan pl;
  if (B <= 0) { set_error("usf_conv_wgrad_wide_f32: %s", B == 0 ? "empty batch" : "bad sizes"); return -2; }
  if (!wide_plan(B, cin, cout, H, W, ks, 0, 0, pl)) return 1;   // shape not served
  if (!x || !dy || !dW || !workspace) { set_error("usf_conv_wgrad_wide_f32: null pointer"); return -1; }
  if (in_act != USF_ACT_NONE && in_act != USF_ACT_LEAKY_RELU) { set_error("usf_conv_wgrad_wide_f32: bad act"); return -2; }
  if (workspace_floats < ((int64_t)pl.slots + kWideReduceRows) * pl.nacc) { set_error("usf_conv_wgrad_wide_f32: workspace too small"); return -2; }
  WwArgs a;
  a.x = x; a.dy = dy; a.part = workspace; a.in_mul = in_mul; a.pre_sub = pre_sub;
  a.B = (int)B; a.cin = (int)cin; a.cout = (int)cout; a.HW = (int)(H * W); a.W = (int)W; a.S = pl.S; a.CSx = pl.CSx; a.CSy = pl.CSy;
  a.q0 = pl.q0; a.nch = pl.nch; a.nex = (int)(cin * H * W); a.ney = (int)(cout * H * W); a.nacc = pl.nacc;
  a.CIT = pl.CIT; a.T = pl.T; a.ntiles = pl.ntiles; a.TG = pl.TG; a.PS = pl.PS; a.lds_floats = pl.lds_floats;
  a.m_hw = wide_magic(a.HW); a.m_w = wide_magic(a.W);
  a.slope_eff = (in_act == USF_ACT_LEAKY_RELU) ? in_slope : 1.f;
  static bool attr_done[USF_MAX_DEVICES][38];
  const int dev = current_device_slot();
  bool launched = false;
#define USF_WW(NT_)                                                                                                        \
  if (pl.NT == NT_) {                                                                                                      \
    const void* fn = reinterpret_cast<const void*>(&conv_wgrad_wide_kernel<NT_>);                                          \
    if (!attr_done[dev][NT_]) {                                                                                            \
      if (hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, kWideLdsMax) != hipSuccess) {                \
        (void)hipGetLastError();                                                                                           \
        set_error("usf_conv_wgrad_wide_f32: cannot raise the kernel's LDS limit");                                        \
        return -3;                                                                                                         \
      }                                                                                                                    \
      attr_done[dev][NT_] = true;                                                                                          \
    }                                                                                                                      \
    hipLaunchKernelGGL((conv_wgrad_wide_kernel<NT_>), dim3((unsigned)pl.blocks), dim3(256), (size_t)pl.lds_bytes, stream, a); \
    launched = true;                                                                                                       \
  }
  USF_WW_INSTANCES(USF_WW)
#undef USF_WW
  if (!launched) { set_error("usf_conv_wgrad_wide_f32: no kernel instance for %d tiles per wave", pl.NT); return -3; }
  int rc = check_launch("usf_conv_wgrad_wide_f32");
  if (rc) return rc;
  const unsigned gx = (unsigned)((pl.nacc + 63) / 64);
  const float* src = workspace;
  int nparts = pl.slots, per, used;
  if (wide_rounds(nparts, per, used) == 2) {
    float* scratch = workspace + (int64_t)pl.slots * pl.nacc;
    hipLaunchKernelGGL(conv_wgrad_wide_sum_kernel, dim3(gx, (unsigned)used), dim3(256), 0, stream, src, nparts, per, pl.nacc, scratch,
                       (float*)nullptr, 0, 0, 0, 0, 0);
    src = scratch;
    nparts = used;
  }
  hipLaunchKernelGGL(conv_wgrad_wide_sum_kernel, dim3(gx, 1u), dim3(256), 0, stream, src, nparts, nparts, pl.nacc, dW, db, 1, (int)cin,
                     (int)cout, pl.CIT, pl.T);
  return check_launch("usf_conv_wgrad_wide_f32 (sum)");
}

// the instantiations the kernel file has (tiles per wave), for usf_conv_wgrad_wide_variant's coverage test
int conv_wgrad_wide_instances(int32_t* out, int32_t cap) {
  const int32_t all[] = {
#define USF_WW_LIST(NT_) NT_,
      USF_WW_INSTANCES(USF_WW_LIST)
#undef USF_WW_LIST
  };
  const int n = (int)(sizeof(all) / sizeof(all[0]));
  for (int i = 0; i < n && i < cap; ++i)
    if (out) out[i] = all[i];
  return n;
}

}  // namespace usf

extern "C" {
int64_t usf_conv_wgrad_wide_workspace(int64_t B, int64_t cin, int64_t cout, int64_t H, int64_t W, int64_t ks) {
  return usf::conv_wgrad_wide_workspace(B, cin, cout, H, W, ks);
}
int usf_conv_wgrad_wide_f32(const float* x, const float* dy, int64_t B, int64_t cin, int64_t cout, int64_t H, int64_t W, int64_t ks,
                            const float* in_mul, const float* pre_sub, int32_t in_act, float in_slope, float* dW, float* db,
                            float* workspace, int64_t workspace_floats, usf_stream_t stream) {
  return usf::conv_wgrad_wide(x, dy, B, cin, cout, H, W, ks, in_mul, pre_sub, in_act, in_slope, dW, db, workspace, workspace_floats,
                              (hipStream_t)stream);
}
int usf_conv_wgrad_wide_variant(const usf_conv_wgrad_query* q, usf_conv_wgrad_wide_info* out) {
  return usf::conv_wgrad_wide_variant(q, out);
}
int usf_conv_wgrad_wide_instances(int32_t* out, int32_t cap) { return usf::conv_wgrad_wide_instances(out, cap); }
}
