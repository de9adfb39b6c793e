// Weight / bias gradient of a stride-1 "same" convolution (kernel 1 or 3) for feature maps of up to 4096 pixels (W <= 64) and
// ANY channel counts up to 64 (usf_conv_wgrad_band_f32): the contract of usf_conv_wgrad_wide_f32 (usf_conv_wgrad_wide.hip)
//     dW[co, ci, tap] = sum_{b, p} dy[b, co, p] * xin[b, ci, p + tap],   db[co] = sum_{b, p} dy[b, co, p],
//     xin = in_act(x - pre_sub[ci]) * in_mul, zeros outside the image,
// exact fp32 on v_mfma_f32_16x16x4_f32 (A = dy[16 co][4 positions], B = x[16 ci][4 shifted positions] -> D[co][ci]).
//
// The wide kernel keeps a whole sample per 256-thread block in LDS, which ends at 256 pixels.  Here the decomposition is the
// same -- x [cinp + 1][CSx] with the row stride S = W + 1, a zero row above and below and a row of ones as db's operand, dy
// [coutp][CSy] with zeros in its pad column, channel strides of 2 * odd, the (cout tile, cin tile, tap) accumulator tiles
// dealt over the four waves, one partial slot per block and position part, fixed-order rounds of the sum -- and what changes
// is the GROUP a persistent block stages: a band of RB consecutive rows of ONE sample, as in usf_conv_band.hip,
//   * x rows r0 - pad .. r0 + RB - 1 + pad and dy rows r0 .. r0 + RB - 1; group g = (sample g / bands, band g % bands);
//   * a block walks its groups in ascending order, the accumulators live across them and leave once.
// What the wide kernel does not have to care about:
//   * a block goes from an interior band to a sample's first or last band, whose halo row lies outside the sample, and to a
//     ragged last band with fewer rows.  EVERY group therefore writes every position of its real channels' image rows -- the
//     value, or an exact zero where the row is outside the sample -- so no group reads what another one staged.  The pad
//     columns, the padding channels and the tail behind the last row are never written after the one clear at the start;
//   * in_mul and pre_sub are applied at the ABSOLUTE pixel c * HW + (r0 - pad + row) * W + col;
//   * a ragged band's MFMA loop ends at its own last chunk; the zeros behind make either choice the same sum;
//   * a block's chains are as long as all its groups' chunks together, so db -- a plain sum, whose fp32 yardstick is torch's
//     pairwise one -- is split over the bias tile's 16 columns (the wide kernel computes the same sum in each of them).
// The element loops find (channel, row, column) with two multiply-high divisions (usf_conv_wgrad_band_plan.h: exact over the
// served range, proven on the CPU by tests/test_conv_wgrad_band_cpu.py from the plan's own magic numbers).
#include "usf_common.h"
#include "usf_conv_wgrad_band_plan.h"

namespace usf {
namespace {

struct WbArgs {
  const float* x;
  const float* dy;
  float* part;             // [slots][nacc]
  const float* in_mul;     // [cin * HW] or NULL
  const float* pre_sub;    // [cin] or NULL
  int cin, cout, H, W, HW, S, CSx, CSy, q0, xbase, pad, nacc;
  int RB, nbands, ngroups, XRW, RBW;     // band rows, bands per sample, B * bands, staged x / dy pixels per channel of a full band
  int CIT, T, ntiles, TG, PS, lds_floats;
  unsigned m_x, m_y, m_w;  // ceil(2^32 / (XRW | RBW | W)); 0: the divisor is 1
  float slope_eff;         // leaky slope of the input nonlinearity; 1 = none
};

__device__ __forceinline__ int wb_div(int e, unsigned magic) { return magic ? (int)__umulhi((unsigned)e, magic) : e; }

template <int NT>
__global__ __launch_bounds__(256) void conv_wgrad_band_kernel(const WbArgs a) {
  extern __shared__ __attribute__((aligned(16))) float wb_lds[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int cinp = a.CIT * 16;
  float* xl = wb_lds;                                           // [cinp][CSx], then the row of ones
  float* dl = wb_lds + (cinp + 1) * a.CSx + kWbOnesLead;        // [coutp][CSy]
  for (int i = tid; i < a.lds_floats; i += 256) wb_lds[i] = 0.f;   // pad columns, padding channels, tails: zero for the whole launch
  __syncthreads();
  // db's operand: ones in the position chunks 0, 16, 32, ... of a row that column j of the bias tile reads from 16 - j chunks
  // in -- column j sums the chunks ch = j (mod 16) alone, sixteen chains a sixteenth as long as one over all chunks, and
  // the last sum adds the columns
  for (int i = tid; i < a.CSx + kWbOnesLead; i += 256) xl[cinp * a.CSx + i] = (i & 63) < 4 ? 1.f : 0.f;

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
        pb[k] = cinp * a.CSx + kWbOnesLead - 4 * (lane & 15) + (lane >> 4);   // the bias tile: D[co][j] = sum of dy[co] over the chunks j (mod 16)
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
  const bool has_ps = a.pre_sub != nullptr, has_mul = a.in_mul != nullptr;
  const int nex = a.cin * a.XRW, ney = a.cout * a.RBW;          // image elements of a full band: every group writes all of them

  for (int g = blockIdx.x; g < a.ngroups; g += gridDim.x) {
    const int smp = g / a.nbands, r0 = (g - smp * a.nbands) * a.RB;
    const int rb = min(a.RB, a.H - r0);                         // rows of this band (a sample's last band may be ragged)
    const int rx0 = r0 - a.pad;                                 // absolute row of the image's first staged x row
    const float* xs = a.x + (int64_t)smp * a.cin * a.HW;
    const float* ys = a.dy + (int64_t)smp * a.cout * a.HW;
    __syncthreads();                                            // the fills / the previous group's fragment reads are done
    for (int e0 = tid; e0 < nex; e0 += 1024) {
      float v[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int e = e0 + 256 * u;
        v[u] = 0.f;
        if (e < nex) {
          const int c = wb_div(e, a.m_x), p = e - c * a.XRW, r = rx0 + wb_div(p, a.m_w);
          if (r >= 0 && r < a.H) v[u] = xs[c * a.HW + rx0 * a.W + p];      // (r * W + col = rx0 * W + p)
        }
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int e = e0 + 256 * u;
        if (e < nex) {
          const int c = wb_div(e, a.m_x), p = e - c * a.XRW, lr = wb_div(p, a.m_w), r = rx0 + lr;
          float val = 0.f;                                      // a row outside the sample: an exact zero, whatever pre_sub is
          if (r >= 0 && r < a.H) {
            val = v[u];
            if (has_ps) val -= a.pre_sub[c];
            val = val > 0.f ? val : val * a.slope_eff;
            if (has_mul) val *= a.in_mul[c * a.HW + rx0 * a.W + p];
          }
          xl[c * a.CSx + a.xbase + p + lr * (a.S - a.W)] = val;
        }
      }
    }
    for (int e0 = tid; e0 < ney; e0 += 1024) {
      float v[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int e = e0 + 256 * u;
        v[u] = 0.f;
        if (e < ney) {
          const int c = wb_div(e, a.m_y), p = e - c * a.RBW;
          if (p < rb * a.W) v[u] = ys[c * a.HW + r0 * a.W + p];
        }
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int e = e0 + 256 * u;
        if (e < ney) {
          const int c = wb_div(e, a.m_y), p = e - c * a.RBW, lr = wb_div(p, a.m_w);
          dl[c * a.CSy + p + lr * (a.S - a.W)] = v[u];          // (rows past a ragged band: the zeros loaded above)
        }
      }
    }
    __syncthreads();
    if (tg < a.ntiles) {
      const int nchg = ((rb - 1) * a.S + a.W + 3) >> 2;         // position chunks up to this band's last pixel
      const int c0 = ps * nchg / a.PS, c1 = (ps + 1) * nchg / a.PS;   // this wave's range of them
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
// then ((0 + 1) + 2) + 3 -- the order of usf_conv_wgrad_wide_f32's rounds.  mode 0: row `by` of out.  mode 1: the slot layout above
// -> dW [cout][cin][T] and db [cout] = the 16 columns of the bias tile added as a fixed tree (the padded channels are dropped).
__global__ __launch_bounds__(256) void conv_wgrad_band_sum_kernel(const float* __restrict__ part, int nparts, int per, int n,
                                                                  float* __restrict__ out, float* __restrict__ out2, int mode, int cin,
                                                                  int cout, int CIT, int T) {
  __shared__ float red[4][64];
  __shared__ float tot[64];
  const int jj = threadIdx.x & 63, g = threadIdx.x >> 6;
  const int j = blockIdx.x * 64 + jj, by = blockIdx.y;
  const int p0 = by * per, p1 = (p0 + per < nparts) ? p0 + per : nparts;
  float s = 0.f;
  if (j < n)
    for (int p = p0 + g; p < p1; p += 4) s += part[(int64_t)p * n + j];
  red[g][jj] = s;
  __syncthreads();
  const float total = ((red[0][jj] + red[1][jj]) + red[2][jj]) + red[3][jj];
  if (mode == 0) {
    if (g == 0 && j < n) out[(int64_t)by * n + j] = total;
    return;
  }
  if (g == 0) tot[jj] = total;
  __syncthreads();
  if (g != 0 || j >= n) return;
  // (T: the taps; a cout tile owns CIT * T weight tiles and behind them its bias tile, whose 16 columns hold db's 16 chains)
  const int tile = j >> 8, r = (j >> 6) & 3, ln = j & 63;
  const int per_cot = CIT * T + 1;
  const int cot = tile / per_cot, rem = tile - cot * per_cot;
  const int co = cot * 16 + 4 * (ln >> 4) + r;
  if (co >= cout) return;
  if (rem == per_cot - 1) {
    if (out2 && (ln & 15) == 0) {
      const float* t = tot + jj;                                // (64 | n: a block's 64 elements are one register of one tile)
      out2[co] = (((t[0] + t[1]) + (t[2] + t[3])) + ((t[4] + t[5]) + (t[6] + t[7]))) +
                 (((t[8] + t[9]) + (t[10] + t[11])) + ((t[12] + t[13]) + (t[14] + t[15])));
    }
    return;
  }
  const int cit = rem / T, t = rem - cit * T;
  const int ci = cit * 16 + (ln & 15);
  if (ci < cin) out[((int64_t)co * cin + ci) * T + t] = total;
}

#define USF_WB_INSTANCES(X) X(1) X(2) X(3) X(4) X(5) X(7) X(8) X(10) X(14) X(15) X(19) X(21) X(28) X(37)

// the plan of a call: the device's compute units where cus <= 0, the grid under the tuning knob conv_wgrad_band_blocks (> 0
// caps it: a test aid, as conv_wgrad_blocks is for usf_conv_wgrad_f32)
bool band_plan(int64_t B, int64_t cin, int64_t cout, int64_t H, int64_t W, int64_t ks, int64_t band_rows, int cus, int blocks_per_cu,
               WbPlan& pl) {
  if (band_rows < 0 || band_rows > 0x7fffffff) return false;
  return wgrad_band_plan(B, cin, cout, H, W, ks, (int)band_rows, cus > 0 ? cus : device_cu_count(), blocks_per_cu,
                         (int)tuning("conv_wgrad_band_blocks", 0), pl);
}

}  // namespace

int conv_wgrad_band_variant(const usf_conv_wgrad_band_query* q, usf_conv_wgrad_band_info* o) {
  if (!q || !o) { set_error("usf_conv_wgrad_band_variant: null pointer"); return -1; }
  *o = usf_conv_wgrad_band_info();
  WbPlan pl;
  if (!band_plan(q->B, q->cin, q->cout, q->H, q->W, q->ks, q->band_rows, q->cus, q->blocks_per_cu, pl)) return 0;
  o->served = 1;
  o->band_rows = pl.RB; o->best_rows = pl.RB_best; o->fit_rows = pl.RB_fit; o->bands = pl.nbands; o->last_rows = pl.last_rows;
  o->groups = pl.groups; o->grid = pl.blocks; o->lds_bytes = pl.lds_bytes;
  o->CIT = pl.CIT; o->COT = pl.COT; o->T = pl.T; o->tiles = pl.ntiles; o->tiles_per_wave = pl.NT; o->wave_groups = pl.TG;
  o->position_parts = pl.PS; o->S = pl.S; o->q0 = pl.q0; o->CSx = pl.CSx; o->CSy = pl.CSy; o->nch = pl.nch; o->nacc = pl.nacc;
  o->slots = pl.slots;
  int per, used;
  o->rounds = wb_rounds(pl.slots, per, used);
  o->per = per;
  o->rows_used = used;
  o->max_groups_per_block = (pl.groups + pl.blocks - 1) / pl.blocks;
  o->blocks_per_cu = pl.per_cu;
  o->cus = pl.cus;
  o->staged_rows = pl.XR;
  o->m_x = pl.m_x; o->m_y = pl.m_y; o->m_w = pl.m_w; o->max_dividend = pl.max_e;
  return 0;
}

int64_t conv_wgrad_band_workspace(int64_t B, int64_t cin, int64_t cout, int64_t H, int64_t W, int64_t ks, int64_t band_rows) {
  WbPlan pl;
  if (!band_plan(B, cin, cout, H, W, ks, band_rows, 0, 0, pl)) return 0;
  return ((int64_t)pl.slots + kWbReduceRows) * pl.nacc;
}

int conv_wgrad_band(const float* x, const float* dy, int64_t B, int64_t cin, int64_t cout, int64_t H, int64_t W, int64_t ks,
                    const float* in_mul, const float* pre_sub, int32_t in_act, float in_slope, float* dW, float* db,
                    float* workspace, int64_t workspace_floats, int64_t band_rows, hipStream_t stream) {
  WbPlan pl;
  if (B <= 0 || band_rows < 0) { set_error("usf_conv_wgrad_band_f32: %s", B == 0 ? "empty batch" : "bad sizes"); return -2; }
  if (!band_plan(B, cin, cout, H, W, ks, band_rows, 0, 0, pl)) return 1;   // shape not served
  if (!x || !dy || !dW || !workspace) { set_error("usf_conv_wgrad_band_f32: null pointer"); return -1; }
  if (in_act != USF_ACT_NONE && in_act != USF_ACT_LEAKY_RELU) { set_error("usf_conv_wgrad_band_f32: bad act"); return -2; }
  if (workspace_floats < ((int64_t)pl.slots + kWbReduceRows) * pl.nacc) { set_error("usf_conv_wgrad_band_f32: workspace too small"); return -2; }
  WbArgs a;
  a.x = x; a.dy = dy; a.part = workspace; a.in_mul = in_mul; a.pre_sub = pre_sub;
  a.cin = (int)cin; a.cout = (int)cout; a.H = (int)H; a.W = (int)W; a.HW = (int)(H * W); a.S = pl.S; a.CSx = pl.CSx; a.CSy = pl.CSy;
  a.q0 = pl.q0; a.xbase = pl.xbase; a.pad = pl.pad; a.nacc = pl.nacc;
  a.RB = pl.RB; a.nbands = pl.nbands; a.ngroups = pl.groups; a.XRW = pl.XR * (int)W; a.RBW = pl.RB * (int)W;
  a.CIT = pl.CIT; a.T = pl.T; a.ntiles = pl.ntiles; a.TG = pl.TG; a.PS = pl.PS; a.lds_floats = pl.lds_floats;
  a.m_x = pl.m_x; a.m_y = pl.m_y; a.m_w = pl.m_w;
  a.slope_eff = (in_act == USF_ACT_LEAKY_RELU) ? in_slope : 1.f;
  static bool attr_done[USF_MAX_DEVICES][38];
  const int dev = current_device_slot();
  bool launched = false;
#define USF_WB(NT_)                                                                                                        \
  if (pl.NT == NT_) {                                                                                                      \
    const void* fn = reinterpret_cast<const void*>(&conv_wgrad_band_kernel<NT_>);                                          \
    if (!attr_done[dev][NT_]) {                                                                                            \
      if (hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, kWbLdsMax) != hipSuccess) {                  \
        (void)hipGetLastError();                                                                                           \
        set_error("usf_conv_wgrad_band_f32: cannot raise the kernel's LDS limit");                                        \
        return -3;                                                                                                         \
      }                                                                                                                    \
      attr_done[dev][NT_] = true;                                                                                          \
    }                                                                                                                      \
    hipLaunchKernelGGL((conv_wgrad_band_kernel<NT_>), dim3((unsigned)pl.blocks), dim3(256), (size_t)pl.lds_bytes, stream, a); \
    launched = true;                                                                                                       \
  }
  USF_WB_INSTANCES(USF_WB)
#undef USF_WB
  if (!launched) { set_error("usf_conv_wgrad_band_f32: no kernel instance for %d tiles per wave", pl.NT); return -3; }
  int rc = check_launch("usf_conv_wgrad_band_f32");
  if (rc) return rc;
  const unsigned gx = (unsigned)((pl.nacc + 63) / 64);
  const float* src = workspace;
  int nparts = pl.slots, per, used;
  if (wb_rounds(nparts, per, used) == 2) {
    float* scratch = workspace + (int64_t)pl.slots * pl.nacc;
    hipLaunchKernelGGL(conv_wgrad_band_sum_kernel, dim3(gx, (unsigned)used), dim3(256), 0, stream, src, nparts, per, pl.nacc, scratch,
                       (float*)nullptr, 0, 0, 0, 0, 0);
    src = scratch;
    nparts = used;
  }
  hipLaunchKernelGGL(conv_wgrad_band_sum_kernel, dim3(gx, 1u), dim3(256), 0, stream, src, nparts, nparts, pl.nacc, dW, db, 1, (int)cin,
                     (int)cout, pl.CIT, pl.T);
  return check_launch("usf_conv_wgrad_band_f32 (sum)");
}

// the instantiations the kernel file has (tiles per wave), for usf_conv_wgrad_band_variant's coverage test
int conv_wgrad_band_instances(int32_t* out, int32_t cap) {
  const int32_t all[] = {
#define USF_WB_LIST(NT_) NT_,
      USF_WB_INSTANCES(USF_WB_LIST)
#undef USF_WB_LIST
  };
  const int n = (int)(sizeof(all) / sizeof(all[0]));
  for (int i = 0; i < n && i < cap; ++i)
    if (out) out[i] = all[i];
  return n;
}

}  // namespace usf

extern "C" {
int64_t usf_conv_wgrad_band_workspace(int64_t B, int64_t cin, int64_t cout, int64_t H, int64_t W, int64_t ks, int64_t band_rows) {
  return usf::conv_wgrad_band_workspace(B, cin, cout, H, W, ks, band_rows);
}
int usf_conv_wgrad_band_f32(const float* x, const float* dy, int64_t B, int64_t cin, int64_t cout, int64_t H, int64_t W, int64_t ks,
                            const float* in_mul, const float* pre_sub, int32_t in_act, float in_slope, float* dW, float* db,
                            float* workspace, int64_t workspace_floats, int64_t band_rows, usf_stream_t stream) {
  return usf::conv_wgrad_band(x, dy, B, cin, cout, H, W, ks, in_mul, pre_sub, in_act, in_slope, dW, db, workspace, workspace_floats,
                              band_rows, (hipStream_t)stream);
}
int usf_conv_wgrad_band_variant(const usf_conv_wgrad_band_query* q, usf_conv_wgrad_band_info* out) {
  return usf::conv_wgrad_band_variant(q, out);
}
int usf_conv_wgrad_band_instances(int32_t* out, int32_t cap) { return usf::conv_wgrad_band_instances(out, cap); }
}
