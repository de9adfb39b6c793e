// The whole backward of a channel-affine layer with FEW channels (the 1 x 1 convolution of BlockAffineTransform behind a
// space-to-depth of a 1- or 3-channel image: C = 4, 12) in ONE launch -- a streaming pass over x and dy:
//
//     dx[b, c', p] = sum_c W[c, c'] * dy[b, c, p]                    W as the forward used it: no transposed copy
//     dW[c, c']    = sum_{b, p} dy[b, c, p] * (x[b, c', p] - pre_sub[c'])
//     db[c]        = sum_{b, p} dy[b, c, p]
//
// The matrix-core weight-gradient kernels pad the channels to 16-wide tiles (C = 4: 1/16 of a tile is useful), stage one sample
// per block per barrier pair and need further launches for dx and for W^T; at a launch-bound batch the number of launches is
// what counts.  Here a thread owns whole pixels: the C^2 + C sums live in its registers, one pixel's (four pixels' in the
// 16-byte form) operands beside them -- 1 <= C <= 12, padded to CP = 4, 8, 12 (channels >= C are never loaded or stored; their
// registers hold zeros).  W and pre_sub sit in LDS, zero-padded: every lane reads the same word (a broadcast).
//
// Arithmetic: fmaf chains in ascending channel order (dx), every thread adds its pixels in ascending order (dW, db: units
// u = block * 256 + thread, + grid * 256, ...; the four pixels of a unit in ascending order), the wave's 64 lanes meet in a
// reduce-scatter of shuffles (per sum: lanes l and l ^ 32 first, then ^ 16, .., ^ 1), the four waves are added through LDS as
// ((0 + 1) + 2) + 3, every block writes ONE slot [dW (C C) | db (C)] and the slots are added by sum_slots (usf_image_grad.hip)
// -- at once or as jobs of usf_partial_sum_jobs_f32.  The grid depends on the sizes (and the form) alone: two runs give the
// same bits.
// dy is read twice per trip (once for dx, once for the sums; the second read hits the cache): the accumulators of dx AND the
// operands of the sums of FOUR pixels at CP = 12 would not fit the register file next to the 156 sums
// (profiles/channel_affine_bwd_resource_usage.md).
// No matrix instructions, no atomics.
#include "usf_common.h"

namespace usf {

int sum_slots(const float* part, int nparts, int n, float* scratch, float* out, usf_psum_job* job, hipStream_t stream, const char* what);
int64_t sum_slots_scratch(int64_t n);
int reduce_rounds(int nparts, int& per, int& used);

constexpr int kCabMaxC = 12;
constexpr int kCabMaxBlocks = 256;          // one block per compute unit of an MI355X; a constant: the grid must not depend on the device

struct CabArgs {
  const float* x; const float* dy; float* dx; const float* W; const float* pre_sub; float* part;
  int64_t units;                              // pixels (scalar form) or groups of four pixels (16-byte form)
  int64_t P;
  int64_t step_b, step_p;                     // the grid's stride (grid * 256 units) in samples and pixels
  int C, slot_floats;
};

template <int PX> struct CabVec;
template <> struct CabVec<1> { typedef float T; };
template <> struct CabVec<4> { typedef f32x4 T; };
__device__ __forceinline__ float cab_get(float v, int) { return v; }
__device__ __forceinline__ float cab_get(const f32x4& v, int j) { return v[j]; }
__device__ __forceinline__ void cab_set(float& v, int, float s) { v = s; }
__device__ __forceinline__ void cab_set(f32x4& v, int j, float s) { v[j] = s; }

// one pixel's / four pixels' values of a channel; a padding channel (on == false, uniform) is not loaded: zeros
template <typename V>
__device__ __forceinline__ V cab_load(const float* p, bool on) {
  V v = V();
  if (on) v = *reinterpret_cast<const V*>(p);
  return v;
}

template <int CP, int PX>
__global__ __launch_bounds__(256) void channel_affine_bwd_kernel(const CabArgs a) {
  typedef typename CabVec<PX>::T V;
  __shared__ float wl[CP * CP + CP];                          // W [CP][CP] zero-padded | pre_sub [CP]
  __shared__ float red[4][CP * CP + CP];
  const int C = a.C;
  for (int i = threadIdx.x; i < CP * CP + CP; i += 256) {
    float v = 0.f;
    if (i < CP * CP) {
      const int r = i / CP, c = i - r * CP;
      if (r < C && c < C) v = a.W[r * C + c];
    } else if (a.pre_sub && i - CP * CP < C) {
      v = a.pre_sub[i - CP * CP];
    }
    wl[i] = v;
  }
  __syncthreads();
  float acc[CP][CP], dbs[CP];
#pragma unroll
  for (int c = 0; c < CP; ++c) {
    dbs[c] = 0.f;
#pragma unroll
    for (int k = 0; k < CP; ++k) acc[c][k] = 0.f;
  }
  // the thread's unit u (a pixel / four pixels of one row) as (sample b, pixel p): one division here, then steps of the grid's
  // stride (step_b samples and step_p pixels, from the host) with a carry -- no division inside the loop
  const int64_t CPs = (int64_t)C * a.P;
  int64_t u = (int64_t)blockIdx.x * 256 + threadIdx.x;
  int64_t b = u * PX / a.P, p = u * PX - b * a.P;
  const int64_t ustep = (int64_t)gridDim.x * 256;
#pragma unroll 1
  for (; u < a.units; u += ustep) {
    const int64_t base = b * CPs + p;
    // W and pre_sub are read from LDS INSIDE the loop: hoisted out of it (they do not change) their CP CP + CP copies would
    // take as many registers again as the sums.  `wv` is `wl` through an offset that is always zero (base < 2^47) but
    // changes with the loop in the compiler's eyes
    const float* wv = wl + (int)(base >> 62);
    b += a.step_b;
    p += a.step_p;
    if (p >= a.P) {
      p -= a.P;
      ++b;
    }
    if (a.dx) {
      V dxv[CP];
#pragma unroll
      for (int k = 0; k < CP; ++k)
#pragma unroll
        for (int j = 0; j < PX; ++j) cab_set(dxv[k], j, 0.f);
#pragma unroll
      for (int c = 0; c < CP; ++c) {
        const V d = cab_load<V>(a.dy + base + (int64_t)c * a.P, c < C);
#pragma unroll
        for (int k = 0; k < CP; ++k) {
          const float w = wv[c * CP + k];
#pragma unroll
          for (int j = 0; j < PX; ++j) cab_set(dxv[k], j, fmaf(w, cab_get(d, j), cab_get(dxv[k], j)));
        }
      }
#pragma unroll
      for (int k = 0; k < CP; ++k)
        if (k < C) *reinterpret_cast<V*>(a.dx + base + (int64_t)k * a.P) = dxv[k];
    }
    V xs[CP];
#pragma unroll
    for (int k = 0; k < CP; ++k) {
      // (a padding channel: 0 - 0, and zero products below -- its sums stay zero and are never stored)
      const V xv = cab_load<V>(a.x + base + (int64_t)k * a.P, k < C);
      const float ps = wv[CP * CP + k];
#pragma unroll
      for (int j = 0; j < PX; ++j) cab_set(xs[k], j, cab_get(xv, j) - ps);
    }
#pragma unroll
    for (int c = 0; c < CP; ++c) {
      const V d = cab_load<V>(a.dy + base + (int64_t)c * a.P, c < C);
#pragma unroll
      for (int j = 0; j < PX; ++j) {
        const float dj = cab_get(d, j);
        dbs[c] += dj;
#pragma unroll
        for (int k = 0; k < CP; ++k) acc[c][k] = fmaf(dj, cab_get(xs[k], j), acc[c][k]);
      }
    }
  }
  // the wave's 64 lanes: a reduce-scatter over the NV = CP CP + CP sums (padded with zeros to a multiple of 64).  At offset
  // o = 32, 16, .., 1 a lane keeps one half of the values it still holds (the upper half when its bit o is set), adds its
  // partner's copy of them and gives the other half away: NV - NV / 64 shuffles where a butterfly per value takes 6 NV; the sum
  // of a value is the butterfly's (lanes l and l ^ 32 first, .. , l ^ 1 last).  Lane l ends with the values R l .. R l + R - 1.
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  constexpr int NV = CP * CP + CP, R = (NV + 63) / 64, NP = 64 * R;
  float v[NP];
#pragma unroll
  for (int e = 0; e < NP; ++e) v[e] = e < CP * CP ? acc[e / CP][e % CP] : e < NV ? dbs[e - CP * CP] : 0.f;
#pragma unroll
  for (int s = 0; s < 6; ++s) {
    const int h = NP >> (s + 1), o = 32 >> s;
    const bool up = (lane & o) != 0;
#pragma unroll
    for (int e = 0; e < h; ++e) {
      const float lo = v[e], hi = v[e + h];
      v[e] = (up ? hi : lo) + __shfl_xor(up ? lo : hi, o, 64);
    }
  }
#pragma unroll
  for (int e = 0; e < R; ++e)
    if (R * lane + e < NV) red[wave][R * lane + e] = v[e];
  __syncthreads();
  // the block's slot [dW (C C) | db (C)]: the four waves in ascending order
  const int t = threadIdx.x;
  if (t < a.slot_floats) {
    const int e = t < C * C ? (t / C) * CP + t % C : CP * CP + (t - C * C);
    a.part[(int64_t)blockIdx.x * a.slot_floats + t] = ((red[0][e] + red[1][e]) + red[2][e]) + red[3][e];
  }
}

// ---- the plan (host only): the launch and the queries below all take it from here ---------------------------------------------
struct CabPlan {
  int served, width, vec, blocks, trips, slot_floats;
  int64_t units;
};

static CabPlan cab_plan(int64_t B, int64_t C, int64_t P, bool vec_ok, bool has_db, int64_t grid_cap) {
  CabPlan pl{};
  if (B < 1 || P < 1 || C < 1 || C > kCabMaxC) return pl;
  if (B > 0x7fffffffffffLL / P / C) return pl;                // (element offsets stay far inside int64)
  pl.served = 1;
  pl.width = (int)((C + 3) / 4 * 4);
  pl.vec = (vec_ok && P % 4 == 0) ? 1 : 0;
  pl.units = pl.vec ? B * P / 4 : B * P;
  const int64_t cap = grid_cap > 0 && grid_cap < kCabMaxBlocks ? grid_cap : kCabMaxBlocks;
  const int64_t want = (pl.units + 255) / 256;
  pl.blocks = (int)(want < cap ? want : cap);
  const int64_t trips = (pl.units + (int64_t)pl.blocks * 256 - 1) / ((int64_t)pl.blocks * 256);
  pl.trips = (int)(trips < 0x7fffffff ? trips : 0x7fffffff);
  pl.slot_floats = (int)(C * C + (has_db ? C : 0));
  return pl;
}

// the tuning aid "channel_affine_bwd_blocks" (> 0: caps the grid below its 256 blocks, so that a small case gives every thread
// several pixels -- tests; 0, the default: the constant cap alone)
static int64_t cab_knob() { return (int64_t)tuning("channel_affine_bwd_blocks", 0); }

int64_t channel_affine_bwd_workspace(int64_t B, int64_t C, int64_t P) {
  // (the scalar form with db: the most blocks and the widest slot a call with these sizes can have)
  const CabPlan pl = cab_plan(B, C, P, false, true, 0);
  if (!pl.served) return 0;
  return (int64_t)pl.blocks * pl.slot_floats + sum_slots_scratch(pl.slot_floats);
}

int channel_affine_bwd_variant(const usf_channel_affine_bwd_query* q, usf_channel_affine_bwd_info* out) {
  if (!q || !out) { set_error("usf_channel_affine_bwd_variant: null pointer"); return -1; }
  *out = usf_channel_affine_bwd_info{};
  const int64_t cap = q->grid_cap > 0 ? q->grid_cap : cab_knob();
  const CabPlan pl = cab_plan(q->B, q->C, q->P, q->aligned16 != 0, q->want_bias != 0, cap);
  if (!pl.served) return 0;
  out->served = 1;
  out->width = pl.width;
  out->vec = pl.vec;
  out->blocks = pl.blocks;
  out->trips = pl.trips;
  out->slot_floats = pl.slot_floats;
  out->slots = pl.blocks;
  int per, used;
  out->rounds = reduce_rounds(pl.blocks, per, used);          // (the rounds sum_slots adds the slots in)
  out->per = per;
  out->rows_used = used;
  out->grid_cap = (int32_t)(cap > 0 && cap < kCabMaxBlocks ? cap : kCabMaxBlocks);
  return 0;
}

int channel_affine_bwd(const float* x, const float* dy, float* dx, int64_t B, int64_t C, int64_t P, const float* W,
                       const float* pre_sub, float* dW, float* db, float* workspace, int64_t workspace_floats, usf_psum_job* job,
                       hipStream_t stream) {
  if (job) job[0].nparts = job[1].nparts = 0;
  if (B == 0 && P >= 1 && C >= 1 && C <= kCabMaxC) return 0;                 // an empty batch: nothing to do
  const bool vec_ok = aligned16(x) && aligned16(dy) && (!dx || aligned16(dx));
  const CabPlan pl = cab_plan(B, C, P, vec_ok, db != nullptr, cab_knob());
  if (!pl.served) return 1;
  if (!x || !dy || !W || !dW) { set_error("usf_channel_affine_bwd_f32: null pointer"); return -1; }
  if (dx == x || dx == dy) { set_error("usf_channel_affine_bwd_f32: in-place operation is not supported"); return -2; }
  if (db && db != dW + C * C) {
    set_error("usf_channel_affine_bwd_f32: db must follow dW (db == dW + C * C: the last sum writes one buffer)");
    return -2;
  }
  if (!workspace || workspace_floats < channel_affine_bwd_workspace(B, C, P)) {
    set_error("usf_channel_affine_bwd_f32: workspace too small (usf_channel_affine_bwd_workspace floats are needed)");
    return -2;
  }
  CabArgs a{};
  a.x = x; a.dy = dy; a.dx = dx; a.W = W; a.pre_sub = pre_sub; a.part = workspace;
  a.units = pl.units; a.P = P; a.C = (int)C; a.slot_floats = pl.slot_floats;
  const int64_t stride = (int64_t)pl.blocks * 256 * (pl.vec ? 4 : 1);           // (pixels)
  a.step_b = stride / P;
  a.step_p = stride % P;
  const dim3 g((unsigned)pl.blocks), bl(256);
#define USF_CAB_LAUNCH(CP_)                                                                                                \
  if (pl.vec) hipLaunchKernelGGL((channel_affine_bwd_kernel<CP_, 4>), g, bl, 0, stream, a);                                \
  else hipLaunchKernelGGL((channel_affine_bwd_kernel<CP_, 1>), g, bl, 0, stream, a);
  switch (pl.width) {
    case 4: USF_CAB_LAUNCH(4) break;
    case 8: USF_CAB_LAUNCH(8) break;
    default: USF_CAB_LAUNCH(12) break;
  }
#undef USF_CAB_LAUNCH
  const int rc = check_launch("usf_channel_affine_bwd_f32");
  if (rc) return rc;
  return sum_slots(workspace, pl.blocks, pl.slot_floats, workspace + (int64_t)pl.blocks * pl.slot_floats, dW, job, stream,
                   "usf_channel_affine_bwd_f32 (sums)");
}

}  // namespace usf
