// Weight / bias gradient of a stride-1 "same" convolution with kernel 5 (usf_conv_wgrad_k5_f32): the contract of
// usf_conv_wgrad_wide_f32 (usf_conv_wgrad_wide.hip)
//     dW[co, ci, tap] = sum_{b, p} dy[b, co, p] * xin[b, ci, p + tap],   db[co] = sum_{b, p} dy[b, co, p],
//     xin = in_act(x - pre_sub[ci]) * in_mul, zeros outside the image,
// exact fp32 on v_mfma_f32_16x16x4_f32 (A = dy[16 co][4 positions], B = x[16 ci][4 shifted positions] -> D[co][ci]), for any
// channel counts up to 64 and maps of up to 256 pixels whose LDS image fits.
//
// The wide kernel's design with the 25 taps DEALT OVER THE GRID: 64 -> 64 channels would need 4 * (4 * 25 + 1) = 404 accumulator
// tiles, 101 per wave -- the register file ends at 37.  So blockIdx.y is a tap ROW (5 taps): a block holds COT * (CIT * 5) weight
// tiles, and the blocks of tap row 0 the COT bias tiles as well (at most 4 * 21 = 84 tiles, 21 per wave).  Every block of a
// column of the grid stages the same samples (x [cinp][CSx], dy [coutp][CSy], channels rounded up to 16 and zero beyond the real
// ones): row stride S = W + 2 with two zero rows above and below the x image, so a tap is a constant offset and a column
// wrap-around of up to two positions lands on a real zero; dy has zeros in its two pad columns, so the padded positions add
// exact zeros.  Channel strides are 2 * odd (bank spread of the ds_read_b32 groups), db rides on a row of ones, as there.
// Tile g of a block belongs to wave g % 4 and is that wave's tile g / 4 (NT tiles per wave, rounded up to an instantiation; a
// slot past the block's last tile repeats the wave's first tile and is never written).  The accumulators live across the
// block's samples and leave once, to the partial slot (tap row, block) owns; a fixed-order sum over each tap row's slots
// follows: same bits on every run, no atomics.
//
// usf_conv_wgrad_k4_f32 is the same kernel at KSZ = 4: four tap rows of four taps in torch's "same" placement (tap (ty, tx) reads
// p + (ty - 1, tx - 1)), 64 -> 64 channels 4 * (4 * 4 + 1) = 68 tiles in tap row 0.  The LDS geometry is the 5 x 5 one: offsets
// -1 .. +2 stay inside the two zero rows and pad columns that -2 .. +2 needs.
#include "usf_common.h"

namespace usf {
namespace {


struct W5Args {
  const float* x;
  const float* dy;
  float* part;             // [tap row][slots][nacc]
  const float* in_mul;     // [cin * HW] or NULL
  const float* pre_sub;    // [cin] or NULL
  int B, HW, W, S, CSx, CSy, q0, nch, nex, ney, nacc, slots;
  int CIT, COT, lds_floats;
  unsigned m_hw, m_w;      // ceil(2^32 / HW), ceil(2^32 / W); 0: the divisor is 1
  float slope_eff;         // leaky slope of the input nonlinearity; 1 = none
};

__device__ __forceinline__ int w5_div(int e, unsigned magic) { return magic ? (int)__umulhi((unsigned)e, magic) : e; }

// KSZ: the kernel size (5 or 4): KSZ tap rows (grid.y) of KSZ taps, the first tap (KSZ - 1) / 2 positions before the pixel
template <int NT, int KSZ>
__global__ __launch_bounds__(256) void conv_wgrad_k5_kernel(const W5Args a) {
  constexpr int kRowTaps = KSZ, kPadB = (KSZ - 1) / 2;
  extern __shared__ __attribute__((aligned(16))) float w5_lds[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int trow = blockIdx.y;                                  // this block's tap row
  const int cinp = a.CIT * 16;
  float* xl = w5_lds;                                           // [cinp][CSx], then the row of ones
  float* dl = w5_lds + (cinp + 1) * a.CSx;                      // [coutp][CSy]
  for (int i = tid; i < a.lds_floats; i += 256) w5_lds[i] = 0.f;   // padding rows, columns and channels: zero for the whole launch
  __syncthreads();
  for (int i = tid; i < a.CSx; i += 256) xl[cinp * a.CSx + i] = 1.f;

  // this wave's tiles: g = wave + 4 k; per cout tile CIT * 5 weight tiles (cin tile, tap of the row) and, in tap row 0, the bias tile
  const int per_cot = a.CIT * kRowTaps + (trow == 0 ? 1 : 0);
  const int ntiles = a.COT * per_cot;
  int pa[NT], pb[NT];
  {
    const int wv = tid >> 6;                                    // (per-lane on purpose: 2 * NT addresses stay in vector registers)
    const int la = (lane & 15) * a.CSy + (lane >> 4);
    const int lb = (lane & 15) * a.CSx + (lane >> 4);
#pragma unroll
    for (int k = 0; k < NT; ++k) {
      const int g = wv + 4 * k;
      const int gg = g < ntiles ? g : wv;
      const int cot = gg / per_cot, rem = gg - cot * per_cot;
      pa[k] = cot * 16 * a.CSy + la;
      if (rem == a.CIT * kRowTaps) {
        pb[k] = cinp * a.CSx + (lane >> 4);                     // the bias tile: B = ones, D[co][*] = sum dy[co]
      } else {
        const int cit = rem / kRowTaps, t = rem - cit * kRowTaps;
        pb[k] = cit * 16 * a.CSx + a.q0 + (trow - kPadB) * a.S + (t - kPadB) + lb;
      }
    }
  }
  f32x4 acc[NT];
#pragma unroll
  for (int k = 0; k < NT; ++k) acc[k] = f32x4{0.f, 0.f, 0.f, 0.f};
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
          const int c = w5_div(e, a.m_hw), p = e - c * a.HW, r = w5_div(p, a.m_w);
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
          const int c = w5_div(e, a.m_hw), p = e - c * a.HW, r = w5_div(p, a.m_w);
          dl[c * a.CSy + p + r * pad] = v[u];
        }
      }
    }
    __syncthreads();
    if (wave < ntiles) {
      for (int ch = 0; ch < a.nch; ++ch) {
#pragma unroll
        for (int k = 0; k < NT; ++k)
          acc[k] = __builtin_amdgcn_mfma_f32_16x16x4f32(dl[pa[k] + 4 * ch], xl[pb[k] + 4 * ch], acc[k], 0, 0, 0);
      }
    }
  }

  // this wave's partial sums: tile g of the tap row at [g * 256 + register * 64 + lane]
  float* pw = a.part + ((int64_t)trow * a.slots + blockIdx.x) * a.nacc;
#pragma unroll
  for (int k = 0; k < NT; ++k) {
    const int g = wave + 4 * k;
    if (g < ntiles) {
#pragma unroll
      for (int r = 0; r < 4; ++r) pw[g * 256 + r * 64 + lane] = acc[k][r];
    }
  }
}

// blockIdx.z = tap row.  out[j] = the sum over the row's partial slots [by * per, min((by + 1) * per, nparts)) in a fixed order:
// four interleaved chains, then ((0 + 1) + 2) + 3 -- the order of usf_conv_wgrad_wide_f32's sum.  mode 0: row `by` of the tap
// row's scratch.  mode 1: the slot layout above -> dW [cout][cin][25] and db [cout] (the padded channels are dropped).
template <int KSZ>
__global__ __launch_bounds__(256) void conv_wgrad_k5_sum_kernel(const float* __restrict__ part, int64_t row_stride, int nparts, int per, int n,
                                                                float* __restrict__ out, int64_t out_row_stride, float* __restrict__ out2,
                                                                int mode, int cin, int cout, int CIT, int COT) {
  constexpr int kTapRows = KSZ, kRowTaps = KSZ;
  __shared__ float red[4][64];
  const int jj = threadIdx.x & 63, g = threadIdx.x >> 6;
  const int j = blockIdx.x * 64 + jj, by = blockIdx.y, trow = blockIdx.z;
  const int p0 = by * per, p1 = (p0 + per < nparts) ? p0 + per : nparts;
  const float* src = part + (int64_t)trow * row_stride;
  const int per_cot = CIT * kRowTaps + (trow == 0 ? 1 : 0);
  const int n_row = COT * per_cot * 256;                        // tap rows 1 .. 4 write fewer tiles than a slot holds: the rest is never read
  float s = 0.f;
  if (j < n_row)
    for (int p = p0 + g; p < p1; p += 4) s += src[(int64_t)p * n + j];
  red[g][jj] = s;
  __syncthreads();
  if (g != 0 || j >= n_row) return;
  const float total = ((red[0][jj] + red[1][jj]) + red[2][jj]) + red[3][jj];
  if (mode == 0) {
    out[(int64_t)trow * out_row_stride + (int64_t)by * n + j] = total;
    return;
  }
  const int tile = j >> 8, r = (j >> 6) & 3, ln = j & 63;
  const int cot = tile / per_cot, rem = tile - cot * per_cot;
  const int co = cot * 16 + 4 * (ln >> 4) + r;
  if (co >= cout) return;
  if (rem == CIT * kRowTaps) {
    if (out2 && (ln & 15) == 0) out2[co] = total;
    return;
  }
  const int cit = rem / kRowTaps, t = rem - cit * kRowTaps;
  const int ci = cit * 16 + (ln & 15);
  if (ci < cin) out[((int64_t)co * cin + ci) * (kTapRows * kRowTaps) + trow * kRowTaps + t] = total;
}

constexpr int kReduceRows = 64;         // scratch rows per tap row of the two-round sum
constexpr int kLdsMax = 160 * 1024;

int k5_rounds(int nparts, int& per, int& used) {
  per = nparts;
  used = 1;
  if (nparts <= 64) return 1;
  const int rows = nparts / 16 < kReduceRows ? (nparts + 15) / 16 : kReduceRows;
  per = (nparts + rows - 1) / rows;
  used = (nparts + per - 1) / per;
  return 2;
}

unsigned k5_magic(int d) { return d < 2 ? 0u : (unsigned)((0x100000000ULL + (unsigned)d - 1) / (unsigned)d); }

int k5_two_odd_at_least(int need) {
  int h = (need + 1) / 2;
  if (!(h & 1)) ++h;
  return 2 * h;
}

#define USF_W5_INSTANCES(X) X(2) X(3) X(6) X(11) X(16) X(21)

struct W5Plan {
  int CIT, COT, S, q0, nch, CSx, CSy, ntiles, NT, nacc, lds_floats, lds_bytes, blocks, slots, per_cu, cus;
};

// KSZ: the entry point's kernel size; ks: what the caller asked for (anything else is not served)
template <int KSZ>
bool k5_plan(int64_t B, int64_t cin, int64_t cout, int64_t H, int64_t W, int64_t ks, int cus, int blocks_per_cu, W5Plan& pl) {
  constexpr int kTapRows = KSZ, kRowTaps = KSZ;
  if (B <= 0 || B > 0x7fffffff || cin <= 0 || cout <= 0 || cin > 64 || cout > 64 || H <= 0 || W <= 0 || H > 256 || W > 256 ||
      H * W > 256 || ks != KSZ)
    return false;
  pl.CIT = (int)(cin + 15) / 16;
  pl.COT = (int)(cout + 15) / 16;
  pl.S = (int)W + 2;
  pl.q0 = 2 * pl.S + 2;
  pl.nch = (int)((H - 1) * pl.S + W + 3) / 4;                    // padded positions from the first to the last pixel, in fours
  pl.CSy = k5_two_odd_at_least(4 * pl.nch);
  pl.CSx = k5_two_odd_at_least(pl.q0 + 4 * pl.nch + 2 * pl.S + 2 + 1);   // last position a fragment read touches + 1
  pl.lds_floats = (pl.CIT * 16 + 1) * pl.CSx + pl.COT * 16 * pl.CSy;
  pl.lds_bytes = pl.lds_floats * 4;
  if (pl.lds_bytes > kLdsMax) return false;
  pl.ntiles = pl.COT * (pl.CIT * kRowTaps + 1);                  // tap row 0, the largest: + one bias tile per cout tile
  const int need = (pl.ntiles + 3) / 4;
  pl.NT = 0;
#define USF_W5_PICK(NT_) if (!pl.NT && need <= NT_) pl.NT = NT_;
  USF_W5_INSTANCES(USF_W5_PICK)
#undef USF_W5_PICK
  if (!pl.NT) return false;
  pl.nacc = pl.ntiles * 256;
  int per_cu = blocks_per_cu > 0 ? blocks_per_cu : kLdsMax / pl.lds_bytes;
  pl.per_cu = per_cu;
  pl.cus = cus > 0 ? cus : device_cu_count();
  // the five tap rows share the compute units: blocks per tap row so that the grid is about one wave of blocks
  int64_t blocks = ((int64_t)pl.cus * (per_cu > 2 ? 2 : per_cu) + kTapRows - 1) / kTapRows;
  if (blocks > B) blocks = B;
  if (blocks < 1) blocks = 1;
  pl.blocks = (int)blocks;
  pl.slots = pl.blocks;
  return true;
}

template <int KSZ> constexpr const char* k5_name() { return KSZ == 5 ? "usf_conv_wgrad_k5" : "usf_conv_wgrad_k4"; }

}  // namespace

template <int KSZ>
int conv_wgrad_k5_variant(const usf_conv_wgrad_query* q, usf_conv_wgrad_wide_info* o) {
  constexpr int kTapRows = KSZ, kRowTaps = KSZ;
  if (!q || !o) { set_error("%s_variant: null pointer", k5_name<KSZ>()); return -1; }
  *o = usf_conv_wgrad_wide_info();
  W5Plan pl;
  if (!k5_plan<KSZ>(q->B, q->cin, q->cout, q->H, q->W, q->ks, q->cus, q->blocks_per_cu, pl)) return 0;
  o->served = 1;
  o->CIT = pl.CIT; o->COT = pl.COT; o->T = kRowTaps; o->tiles = pl.ntiles; o->tiles_per_wave = pl.NT; o->wave_groups = 4;
  o->position_parts = kTapRows; o->blocks = pl.blocks; o->lds_bytes = pl.lds_bytes; o->S = pl.S; o->q0 = pl.q0; o->CSx = pl.CSx;
  o->CSy = pl.CSy; o->nch = pl.nch; o->nacc = pl.nacc; o->slots = pl.slots;
  int per, used;
  o->rounds = k5_rounds(pl.slots, per, used);
  o->per = per;
  o->rows_used = used;
  o->max_samples_per_block = (int32_t)((q->B + pl.blocks - 1) / pl.blocks);
  o->blocks_per_cu = pl.per_cu;
  o->cus = pl.cus;
  return 0;
}

template <int KSZ>
int64_t conv_wgrad_k5_workspace(int64_t B, int64_t cin, int64_t cout, int64_t H, int64_t W, int64_t ks) {
  constexpr int kTapRows = KSZ;
  W5Plan pl;
  if (!k5_plan<KSZ>(B, cin, cout, H, W, ks, 0, 0, pl)) return 0;
  return (int64_t)kTapRows * ((int64_t)pl.slots + kReduceRows) * pl.nacc;
}

template <int KSZ>
int conv_wgrad_k5(const float* x, const float* dy, int64_t B, int64_t cin, int64_t cout, int64_t H, int64_t W, int64_t ks,
                  const float* in_mul, const float* pre_sub, int32_t in_act, float in_slope, float* dW, float* db, float* workspace,
                  int64_t workspace_floats, hipStream_t stream) {
  constexpr int kTapRows = KSZ;
  W5Plan pl;
  if (B <= 0) { set_error("%s_f32: %s", k5_name<KSZ>(), B == 0 ? "empty batch" : "bad sizes"); return -2; }
  if (!k5_plan<KSZ>(B, cin, cout, H, W, ks, 0, 0, pl)) return 1;     // shape not served
  if (!x || !dy || !dW || !workspace) { set_error("%s_f32: null pointer", k5_name<KSZ>()); return -1; }
  if (in_act != USF_ACT_NONE && in_act != USF_ACT_LEAKY_RELU) { set_error("%s_f32: bad act", k5_name<KSZ>()); return -2; }
  if (workspace_floats < (int64_t)kTapRows * ((int64_t)pl.slots + kReduceRows) * pl.nacc) {
    set_error("%s_f32: workspace too small", k5_name<KSZ>());
    return -2;
  }
  W5Args a;
  a.x = x; a.dy = dy; a.part = workspace; a.in_mul = in_mul; a.pre_sub = pre_sub;
  a.B = (int)B; a.HW = (int)(H * W); a.W = (int)W; a.S = pl.S; a.CSx = pl.CSx; a.CSy = pl.CSy;
  a.q0 = pl.q0; a.nch = pl.nch; a.nex = (int)(cin * H * W); a.ney = (int)(cout * H * W); a.nacc = pl.nacc; a.slots = pl.slots;
  a.CIT = pl.CIT; a.COT = pl.COT; a.lds_floats = pl.lds_floats;
  a.m_hw = k5_magic(a.HW); a.m_w = k5_magic(a.W);
  a.slope_eff = (in_act == USF_ACT_LEAKY_RELU) ? in_slope : 1.f;
  static bool attr_done[USF_MAX_DEVICES][22];                  // (one table per KSZ: this function is a template)
  const int dev = current_device_slot();
  bool launched = false;
#define USF_W5(NT_)                                                                                                          \
  if (pl.NT == NT_) {                                                                                                        \
    const void* fn = reinterpret_cast<const void*>(&conv_wgrad_k5_kernel<NT_, KSZ>);                                         \
    if (!attr_done[dev][NT_]) {                                                                                              \
      if (hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, kLdsMax) != hipSuccess) {                      \
        (void)hipGetLastError();                                                                                             \
        set_error("%s_f32: cannot raise the kernel's LDS limit", k5_name<KSZ>());                                           \
        return -3;                                                                                                           \
      }                                                                                                                      \
      attr_done[dev][NT_] = true;                                                                                            \
    }                                                                                                                        \
    hipLaunchKernelGGL((conv_wgrad_k5_kernel<NT_, KSZ>), dim3((unsigned)pl.blocks, (unsigned)kTapRows), dim3(256), (size_t)pl.lds_bytes, \
                       stream, a);                                                                                           \
    launched = true;                                                                                                         \
  }
  USF_W5_INSTANCES(USF_W5)
#undef USF_W5
  if (!launched) { set_error("%s_f32: no kernel instance for %d tiles per wave", k5_name<KSZ>(), pl.NT); return -3; }
  int rc = check_launch(KSZ == 5 ? "usf_conv_wgrad_k5_f32" : "usf_conv_wgrad_k4_f32");
  if (rc) return rc;
  const unsigned gx = (unsigned)((pl.nacc + 63) / 64);
  const float* src = workspace;
  int64_t src_stride = (int64_t)pl.slots * pl.nacc;
  int nparts = pl.slots, per, used;
  if (k5_rounds(nparts, per, used) == 2) {
    float* scratch = workspace + (int64_t)kTapRows * pl.slots * pl.nacc;
    hipLaunchKernelGGL(conv_wgrad_k5_sum_kernel<KSZ>, dim3(gx, (unsigned)used, (unsigned)kTapRows), dim3(256), 0, stream, src, src_stride, nparts,
                       per, pl.nacc, scratch, (int64_t)kReduceRows * pl.nacc, (float*)nullptr, 0, 0, 0, pl.CIT, pl.COT);
    src = scratch;
    src_stride = (int64_t)kReduceRows * pl.nacc;
    nparts = used;
  }
  hipLaunchKernelGGL(conv_wgrad_k5_sum_kernel<KSZ>, dim3(gx, 1u, (unsigned)kTapRows), dim3(256), 0, stream, src, src_stride, nparts, nparts,
                     pl.nacc, dW, (int64_t)0, db, 1, (int)cin, (int)cout, pl.CIT, pl.COT);
  return check_launch(KSZ == 5 ? "usf_conv_wgrad_k5_f32 (sum)" : "usf_conv_wgrad_k4_f32 (sum)");
}

// the instantiations the kernel file has (tiles per wave), for usf_conv_wgrad_k5_variant's coverage test
int conv_wgrad_k5_instances(int32_t* out, int32_t cap) {
  const int32_t all[] = {
#define USF_W5_LIST(NT_) NT_,
      USF_W5_INSTANCES(USF_W5_LIST)
#undef USF_W5_LIST
  };
  const int n = (int)(sizeof(all) / sizeof(all[0]));
  for (int i = 0; i < n && i < cap; ++i)
    if (out) out[i] = all[i];
  return n;
}

}  // namespace usf

extern "C" {
int64_t usf_conv_wgrad_k5_workspace(int64_t B, int64_t cin, int64_t cout, int64_t H, int64_t W, int64_t ks) {
  return usf::conv_wgrad_k5_workspace<5>(B, cin, cout, H, W, ks);
}
int usf_conv_wgrad_k5_f32(const float* x, const float* dy, int64_t B, int64_t cin, int64_t cout, int64_t H, int64_t W, int64_t ks,
                          const float* in_mul, const float* pre_sub, int32_t in_act, float in_slope, float* dW, float* db,
                          float* workspace, int64_t workspace_floats, usf_stream_t stream) {
  return usf::conv_wgrad_k5<5>(x, dy, B, cin, cout, H, W, ks, in_mul, pre_sub, in_act, in_slope, dW, db, workspace, workspace_floats,
                               (hipStream_t)stream);
}
int usf_conv_wgrad_k5_variant(const usf_conv_wgrad_query* q, usf_conv_wgrad_wide_info* out) { return usf::conv_wgrad_k5_variant<5>(q, out); }
int usf_conv_wgrad_k5_instances(int32_t* out, int32_t cap) { return usf::conv_wgrad_k5_instances(out, cap); }
int64_t usf_conv_wgrad_k4_workspace(int64_t B, int64_t cin, int64_t cout, int64_t H, int64_t W, int64_t ks) {
  return usf::conv_wgrad_k5_workspace<4>(B, cin, cout, H, W, ks);
}
int usf_conv_wgrad_k4_f32(const float* x, const float* dy, int64_t B, int64_t cin, int64_t cout, int64_t H, int64_t W, int64_t ks,
                          const float* in_mul, const float* pre_sub, int32_t in_act, float in_slope, float* dW, float* db,
                          float* workspace, int64_t workspace_floats, usf_stream_t stream) {
  return usf::conv_wgrad_k5<4>(x, dy, B, cin, cout, H, W, ks, in_mul, pre_sub, in_act, in_slope, dW, db, workspace, workspace_floats,
                               (hipStream_t)stream);
}
int usf_conv_wgrad_k4_variant(const usf_conv_wgrad_query* q, usf_conv_wgrad_wide_info* out) { return usf::conv_wgrad_k5_variant<4>(q, out); }
int usf_conv_wgrad_k4_instances(int32_t* out, int32_t cap) { return usf::conv_wgrad_k5_instances(out, cap); }
}
