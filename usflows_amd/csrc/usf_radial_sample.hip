// RadialDistribution.sample (src/usflows/distributions.py:474-499) in ONE launch: the radius from the norm distribution AND the
// direction on the unit Lp sphere, both pure functions of (seed, offset, row + row_offset, parameters).
//   r ~ norm_distribution -- the K-component mixtures (K <= 64) of LogNormal / Gamma / Weibull / HalfNormal / Chi components that
//       usf_radial_logprob_f32 evaluates (usf_radial.hip), with the same parameter conventions (stored through softplus unless
//       USF_NORM_RAW_PARAMS; Chi raw only; HalfNormal without par_b)
//   z = loc + r * u,  u uniform on the unit Lp sphere: usf_radial_sample_f32's counters, streams and arithmetic, unchanged
//       (usf_elementwise.hip: radial_sample_kernel) -- z is bit for bit what that kernel writes when handed this kernel's r_out.
// The torch formulation draws r from torch's global generator through a validating distribution object (a host read-back per call):
// not reproducible from a seed, not invariant under a split of the rows over launches or ranks, not capturable.
// One wave per row, four rows per block.  HBM-bound at the z rows it writes; the radius is O(K + attempts) fp64 work per row that
// every lane computes uniformly (no divergence, no cross-lane traffic but one ballot for the component).  No atomics.
#include "usf_common.h"

namespace usf {

constexpr int RSM_MAXK = 64;               // = RAD_MAXK of usf_radial.hip
constexpr int RSM_WPB = 4;                 // waves (rows in flight) per block
constexpr int RSM_GAMMA_ATTEMPTS = 32;     // Marsaglia-Tsang rejection loop: a COMPILE-TIME bound (acceptance >= 0.95 per attempt)
constexpr uint64_t RSM_STREAM = 0x85ebca6bu;       // the radius draws' Philox stream: offset ^ RSM_STREAM ^ (attempt << 32)
constexpr uint32_t RSM_BOOST_ATTEMPT = 0xFFFFu;    // the "attempt" whose word 0 is the a < 1 boost's uniform

// Philox4x32-10 and the fp32 word -> variate map, exactly as usf_elementwise.hip has them (the direction draw must not differ)
__device__ __forceinline__ void philox_round(uint32_t (&c)[4], uint32_t k0, uint32_t k1) {
  const uint64_t p0 = (uint64_t)0xD2511F53u * c[0];
  const uint64_t p1 = (uint64_t)0xCD9E8D57u * c[2];
  const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c[1] ^ k0;
  const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c[3] ^ k1;
  c[0] = n0; c[1] = (uint32_t)p1; c[2] = n2; c[3] = (uint32_t)p0;
}
__device__ __forceinline__ void philox4x32_10(uint64_t ctr, uint64_t stream_id, uint64_t seed, uint32_t (&out)[4]) {
  uint32_t c[4] = {(uint32_t)ctr, (uint32_t)(ctr >> 32), (uint32_t)stream_id, (uint32_t)(stream_id >> 32)};
  uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    philox_round(c, k0, k1);
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
  out[0] = c[0]; out[1] = c[1]; out[2] = c[2]; out[3] = c[3];
}
__device__ __forceinline__ float u01(uint32_t x) { return ((float)(x >> 9) + 0.5f) * (1.0f / 8388608.0f); }

// the radius draw's uniform: all 32 bits at the cell centres (w + 1/2) * 2^-32 -- exact in fp64, never 0 or 1
__device__ __forceinline__ double u01_d(uint32_t w) { return ((double)w + 0.5) * (1.0 / 4294967296.0); }
// Box-Muller, the cosine branch
__device__ __forceinline__ double normal_d(uint32_t w1, uint32_t w2) {
  return sqrt(-2.0 * log(u01_d(w1))) * cos(6.28318530717958647692 * u01_d(w2));
}
__device__ __forceinline__ double softplus_d(double x) { return x > 20.0 ? x : log1p(exp(x)); }

// per-component constants, one set per block in LDS
struct RsmTab {
  double a[RSM_MAXK];      // LogNormal: mu      Gamma: concentration      Weibull: scale              HalfNormal: sigma      Chi: df
  double b[RSM_MAXK];      // LogNormal: sigma   Gamma: rate               Weibull: concentration                             Chi: scale
  double cum[RSM_MAXK];    // C_j = sum_{i <= j} exp(l_i - max l), added in index order (1 when there are no logits)
};

// called by the first wave of a block (all 64 lanes); others wait at the barrier that follows
__device__ __forceinline__ void build_sample_tab(RsmTab& t, int norm, int K, const float* __restrict__ par_a,
                                                 const float* __restrict__ par_b, const float* __restrict__ logits, int lane) {
  const bool raw = (norm & USF_NORM_RAW_PARAMS) != 0;
  const int kind = norm & 0xff;
  const bool on = lane < K;
  double cum = 1.0;
  if (logits) {
    const double l = on ? (double)logits[lane] : -INFINITY;
    double mx = l;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) mx = fmax(mx, __shfl_xor(mx, o, 64));
    const double e = on ? exp(l - mx) : 0.0;
    cum = 0.0;
    for (int i = 0; i < K; ++i) {                       // (the same left-to-right sum in every lane that keeps it)
      const double ei = __shfl(e, i, 64);
      if (i <= lane) cum += ei;
    }
  }
  if (on) {
    const double pa = (double)par_a[lane], pb = par_b ? (double)par_b[lane] : 1.0;      // (one-parameter kinds: no par_b)
    double a, b;
    if (kind == USF_NORM_LOGNORMAL) {
      a = pa;
      b = raw ? pb : softplus_d(pb);
    } else if (kind == USF_NORM_GAMMA || kind == USF_NORM_WEIBULL) {
      a = raw ? pa : softplus_d(pa);
      b = raw ? pb : softplus_d(pb);
    } else if (kind == USF_NORM_HALFNORMAL) {
      a = raw ? pa : softplus_d(pa);
      b = 1.0;
    } else {                                            // USF_NORM_CHI: df and the constant scale, always as they are
      a = pa;
      b = pb;
    }
    t.a[lane] = a; t.b[lane] = b; t.cum[lane] = cum;
  }
}

// Gamma(shape, 1) by Marsaglia & Tsang (2000) over the attempts' Philox blocks; `first` = attempt 0's block (already drawn)
__device__ __forceinline__ double gamma_draw_d(double shape, uint64_t ctr, uint64_t stream0, uint64_t seed, const uint32_t (&first)[4]) {
  const double a1 = shape < 1.0 ? shape + 1.0 : shape;
  const double d = a1 - 1.0 / 3.0, c = 1.0 / sqrt(9.0 * d);
  double g = d;                                         // (no attempt accepted: unreachable in practice, and no spin)
  uint32_t w[4] = {first[0], first[1], first[2], first[3]};
#pragma unroll 1
  for (int t = 0; t < RSM_GAMMA_ATTEMPTS; ++t) {
    if (t > 0) philox4x32_10(ctr, stream0 ^ ((uint64_t)t << 32), seed, w);
    const double n = normal_d(w[1], w[2]);
    const double q = 1.0 + c * n;
    const double v = q * q * q;
    if (v > 0.0 && log(u01_d(w[3])) < 0.5 * n * n + d - d * v + d * log(v)) {
      g = d * v;
      break;
    }
  }
  if (shape < 1.0) {
    philox4x32_10(ctr, stream0 ^ ((uint64_t)RSM_BOOST_ATTEMPT << 32), seed, w);
    g *= pow(u01_d(w[0]), 1.0 / shape);
  }
  return g;
}

// the radius of counter `ctr`, the same value in every lane of the wave
__device__ __forceinline__ float draw_radius(const RsmTab& tab, int kind, int K, bool mix, uint64_t ctr, uint64_t offset, uint64_t seed,
                                             int lane) {
  const uint64_t stream0 = offset ^ RSM_STREAM;
  uint32_t w[4];
  philox4x32_10(ctr, stream0, seed, w);
  int k = 0;
  if (mix) {
    const double t = u01_d(w[0]) * tab.cum[K - 1];
    k = __popcll(__ballot(lane < K && tab.cum[lane < K ? lane : 0] <= t));
    k = k < K - 1 ? k : K - 1;
  }
  const double a = tab.a[k], b = tab.b[k];
  double r;
  if (kind == USF_NORM_LOGNORMAL) r = exp(a + b * normal_d(w[1], w[2]));
  else if (kind == USF_NORM_HALFNORMAL) r = a * fabs(normal_d(w[1], w[2]));
  else if (kind == USF_NORM_WEIBULL) r = a * pow(-log(u01_d(w[1])), 1.0 / b);
  else if (kind == USF_NORM_GAMMA) r = gamma_draw_d(a, ctr, stream0, seed, w) / b;
  else r = b * sqrt(2.0 * gamma_draw_d(0.5 * a, ctr, stream0, seed, w));
  r = fmax(r, 1.17549435082228750797e-38);             // the smallest normal fp32, as torch's Gamma.rsample clamps
  return (float)r;
}

__global__ __launch_bounds__(64 * RSM_WPB) void radial_sample_norm_kernel(
    float* __restrict__ z, int64_t ldz, int64_t M, int D, int base, const float* __restrict__ loc, int norm, int K,
    const float* __restrict__ par_a, const float* __restrict__ par_b, const float* __restrict__ logits, float* __restrict__ r_out,
    uint64_t seed, uint64_t offset, int64_t row_offset) {
  __shared__ RsmTab tab;
  const int lane = threadIdx.x & 63, wib = threadIdx.x >> 6;
  if (wib == 0) build_sample_tab(tab, norm, K, par_a, par_b, logits, lane);
  __syncthreads();
  const int kind = norm & 0xff;
  const bool mix = logits != nullptr && K > 1;
  const int64_t groups_per_row = (D + 3) / 4;
  for (int64_t m = (int64_t)blockIdx.x * RSM_WPB + wib; m < M; m += (int64_t)gridDim.x * RSM_WPB) {
    const float rf = draw_radius(tab, kind, K, mix, (uint64_t)(m + row_offset), offset, seed, lane);
    if (r_out && lane == 0) r_out[m] = rf;
    if (!z) continue;
    // ---- the direction: radial_sample_kernel (usf_elementwise.hip) with mul = rf ----
    float* zr = z + m * ldz;
    float acc = 0.f;
    // pass 1: raw variates into the row, reduction of the normaliser
    for (int64_t g = lane; g < groups_per_row; g += 64) {
      uint32_t rnd[4], rnd2[4];
      philox4x32_10((uint64_t)((m + row_offset) * groups_per_row + g), offset, seed, rnd);
      float v[4];
      if (base == USF_BASE_LPNORM1) {
        philox4x32_10((uint64_t)((m + row_offset) * groups_per_row + g), offset ^ 0x5bd1e995u, seed, rnd2);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const float e = -logf(u01(rnd[j]));
          acc += ((int)(g * 4 + j) < D) ? e : 0.f;
          v[j] = (rnd2[j] & 1u) ? e : -e;
        }
      } else if (base == USF_BASE_LPNORM2) {
        const float r0 = sqrtf(-2.0f * logf(u01(rnd[0]))), r1 = sqrtf(-2.0f * logf(u01(rnd[2])));
        float s0, c0, s1, c1;
        sincosf(6.28318530717958647692f * u01(rnd[1]), &s0, &c0);
        sincosf(6.28318530717958647692f * u01(rnd[3]), &s1, &c1);
        v[0] = r0 * c0; v[1] = r0 * s0; v[2] = r1 * c1; v[3] = r1 * s1;
#pragma unroll
        for (int j = 0; j < 4; ++j) acc += ((int)(g * 4 + j) < D) ? v[j] * v[j] : 0.f;
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = 2.0f * u01(rnd[j]) - 1.0f;
      }
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if ((int)(g * 4 + j) < D) zr[g * 4 + j] = v[j];
    }
    acc = wave_sum(acc);
    float mul = rf;
    int extremal = -1;
    if (base == USF_BASE_LPNORM1) mul = mul / acc;
    else if (base == USF_BASE_LPNORM2) mul = mul / sqrtf(acc);
    else {
      uint32_t rnd[4];
      philox4x32_10((uint64_t)(m + row_offset), offset ^ 0x9e3779b9u, seed, rnd);
      extremal = (int)(((uint64_t)rnd[0] * (uint64_t)D) >> 32);     // uniform index in [0, D)
    }
    // pass 2: each lane rescales the elements it wrote itself (no cross-lane dependency on memory)
    for (int64_t g = lane; g < groups_per_row; g += 64)
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int d = (int)(g * 4 + j);
        if (d < D) zr[d] = loc[d] + mul * (d == extremal ? 1.0f : zr[d]);
      }
  }
}

int radial_sample_norm(float* z, int64_t ldz, int64_t M, int64_t D, int32_t p_id, const float* loc, int32_t norm, int32_t K,
                       const float* par_a, const float* par_b, const float* logits, float* r_out, uint64_t seed, uint64_t offset,
                       int64_t row_offset, hipStream_t stream) {
  const char* what = "usf_radial_sample_norm_f32";
  if (M < 0 || M > 0x7fffffff || (z && (D <= 0 || D > 0x7fffffff || ldz < D))) { set_error("%s: bad sizes", what); return -2; }
  if (z && p_id != USF_BASE_LPNORM1 && p_id != USF_BASE_LPNORM2 && p_id != USF_BASE_LPNORMINF) {
    set_error("%s: p id %d is not an Lp-radial id", what, p_id);
    return -2;
  }
  const int kind = norm & 0xff;
  if (kind < USF_NORM_LOGNORMAL || kind > USF_NORM_CHI || (norm & ~(0xff | USF_NORM_RAW_PARAMS))) {
    set_error("%s: unknown norm-distribution id %d", what, norm);
    return -2;
  }
  if (kind == USF_NORM_CHI && !(norm & USF_NORM_RAW_PARAMS)) {
    set_error("%s: USF_NORM_CHI takes df and scale as they are (USF_NORM_RAW_PARAMS)", what);
    return -2;
  }
  if (K < 1 || K > RSM_MAXK) { set_error("%s: K = %d components (1..%d served)", what, K, RSM_MAXK); return -2; }
  if (M == 0) return 0;
  if ((z && !loc) || (!z && !r_out) || !par_a || (!par_b && kind != USF_NORM_HALFNORMAL) || (K > 1 && !logits)) {
    set_error("%s: null pointer", what);
    return -1;
  }
  int64_t blocks = (M + RSM_WPB - 1) / RSM_WPB;
  if (blocks > 256 * 16) blocks = 256 * 16;
  hipLaunchKernelGGL(radial_sample_norm_kernel, dim3((unsigned)blocks), dim3(64 * RSM_WPB), 0, stream, z, ldz, M, z ? (int)D : 0,
                     (int)p_id, loc, (int)norm, (int)K, par_a, par_b, logits, r_out, seed, offset, row_offset);
  return check_launch(what);
}

}  // namespace usf
