// Shared device/host helpers for libusflows_hip.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/usflows_hip_internal.h"

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));

#define USF_WAVE 64

namespace usf {

void set_error(const char* fmt, ...);
// a named tuning knob (usf_api.hip: the one table, preset from USFLOWS_AMD_TUNE, changed with usf_set_tuning)
long long tuning(const char* name, long long dflt);
// measurement aid (usf_set_clock_buffer): device buffer [2] that the planes GEMM and the MFMA probe add their blocks' lifetimes
// to -- [0] shader-clock cycles (s_memtime), [1] ticks of the constant 100 MHz counter (s_memrealtime); nullptr: off
unsigned long long* clock_buffer();

static inline int check_launch(const char* what) {
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    set_error("%s: launch failed: %s", what, hipGetErrorString(e));
    return (int)e;
  }
  return 0;
}

static inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

// Per-device launch state (a process may drive several GPUs: function attributes and the CU count belong to a device)
#define USF_MAX_DEVICES 64
static inline int current_device_slot() {
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= USF_MAX_DEVICES) dev = 0;
  return dev;
}
// compute units of the current device (cached per device; 256 when the query fails)
static inline int device_cu_count() {
  static int cus[USF_MAX_DEVICES] = {0};
  const int dev = current_device_slot();
  if (cus[dev] <= 0) {
    hipDeviceProp_t prop;
    cus[dev] = (hipGetDeviceProperties(&prop, dev) == hipSuccess && prop.multiProcessorCount > 0) ? prop.multiProcessorCount : 256;
  }
  return cus[dev];
}

// leaky_relu exactly as ATen: x > 0 ? x : x * slope
__device__ __forceinline__ float act_apply(float v, int act, float slope) {
  return (act == USF_ACT_LEAKY_RELU) ? (v > 0.0f ? v : v * slope) : v;
}
// USF_ACT_GATE: leaky_relu_backward from the saved OUTPUT h (as usf_act_grad_f32: h > 0 ? v : v * slope)
__device__ __forceinline__ float gate_apply(float v, float h, float slope) { return (h > 0.0f) ? v : v * slope; }

// The vector context of usf_coupling_additive_vctx_f32 (usflows_hip_internal.h), validated by coupling_dispatch; nullptr or
// ctx == nullptr: no vector context
struct CplVctx {
  const float* ctx; int64_t ld_ctx; int ctx_dim;
  const float* W_ctx_t; int64_t ldw_ctx; const float* b_ctx;
};
// X[ht][t] += b_ctx[h] + sum_{c < C} ctx[row, c] * W_ctx_t[c, h]  for h = 16 ht + 4 lg + t: the accumulator layout of the fused
// coupling kernels (a lane's four consecutive hidden units = one 16-byte load per context column).  The sum runs over c in
// ascending order in fp32 and is added to the pre-activation as ONE term (networks.py:741-743: layers[0](x) + layers[1](context)).
// crow: the row's context columns, 16-byte aligned; whole groups of four are loaded, so the padding columns [C, round_up(C, 4))
// are read but never enter the arithmetic.  Four hidden tiles at a time: 16 running sums, the weight loads of a group of four
// columns in flight together.
template <int T>
__device__ __forceinline__ void vctx_add(f32x4 (&X)[T], const float* crow, int C, const float* Wt, int64_t ldw, const float* bc,
                                         int lg) {
  constexpr int G = T < 4 ? T : 4;
#pragma unroll
  for (int h0 = 0; h0 < T; h0 += G) {
    f32x4 s[G];
#pragma unroll
    for (int i = 0; i < G; ++i) s[i] = *reinterpret_cast<const f32x4*>(bc + (h0 + i) * 16 + 4 * lg);
    const float* w = Wt + h0 * 16 + 4 * lg;
    int c = 0;
#pragma unroll 1
    for (; c + 4 <= C; c += 4) {
      const f32x4 cv = *reinterpret_cast<const f32x4*>(crow + c);
#pragma unroll
      for (int e = 0; e < 4; ++e)
#pragma unroll
        for (int i = 0; i < G; ++i) s[i] += cv[e] * *reinterpret_cast<const f32x4*>(w + (int64_t)(c + e) * ldw + 16 * i);
    }
    if (c < C) {
      const f32x4 cv = *reinterpret_cast<const f32x4*>(crow + c);
#pragma unroll
      for (int e = 0; e < 3; ++e)
        if (c + e < C) {
#pragma unroll
          for (int i = 0; i < G; ++i) s[i] += cv[e] * *reinterpret_cast<const f32x4*>(w + (int64_t)(c + e) * ldw + 16 * i);
        }
    }
#pragma unroll
    for (int i = 0; i < G; ++i) X[h0 + i] += s[i];
  }
}

// The context channel of a conditional conditioner's first convolution (usf_conv2d_same_ctx_f32): a constant plane ctx[b]
// under zero padding contributes ctx[b] * S[co, p] with S = the sum of the channel's taps that land inside the image at p.
// ctx_tapmask: bit t (t = dy * ks + dx) set when tap t of output pixel (py, px) reads inside the H x W image.
__host__ __device__ __forceinline__ unsigned ctx_tapmask(int py, int px, int H, int W, int ks) {
  if (ks == 1) return 1u;
  const unsigned rowok = (py > 0 ? 0x007u : 0u) | 0x038u | (py + 1 < H ? 0x1c0u : 0u);
  const unsigned colok = (px > 0 ? 0x049u : 0u) | 0x092u | (px + 1 < W ? 0x124u : 0u);
  return rowok & colok;
}
// ks = 5: 25 bits; a row / column of taps is inside at distance 0, 1 or >= 2 from each border (H or W below 3: both borders at
// once).  A function of its own, chosen at compile time by the 5 x 5 instantiations: the ks = 1 / 3 callers compile as before.
__host__ __device__ __forceinline__ unsigned ctx_tapmask5(int py, int px, int H, int W) {
  unsigned rows = 0u, cols = 0u;
#pragma unroll
  for (int d = 0; d < 5; ++d) {
    rows |= ((unsigned)(py + d - 2) < (unsigned)H ? 1u : 0u) << (5 * d);     // bit 5 d: tap row d reads inside
    cols |= ((unsigned)(px + d - 2) < (unsigned)W ? 1u : 0u) << d;
  }
  return rows * cols;                                                        // (no carries: cols < 32)
}
// ks = 4 in torch's "same" placement (one zero before, two after): 16 bits, bit dy * 4 + dx set when 0 <= py + dy - 1 < H and
// 0 <= px + dx - 1 < W.  Chosen at compile time by the 4 x 4 instantiations, as ctx_tapmask5 by the 5 x 5 ones.
__host__ __device__ __forceinline__ unsigned ctx_tapmask4(int py, int px, int H, int W) {
  unsigned rows = 0u, cols = 0u;
#pragma unroll
  for (int d = 0; d < 4; ++d) {
    rows |= ((unsigned)(py + d - 1) < (unsigned)H ? 1u : 0u) << (4 * d);     // bit 4 d: tap row d reads inside
    cols |= ((unsigned)(px + d - 1) < (unsigned)W ? 1u : 0u) << d;
  }
  return rows * cols;                                                        // (no carries: cols < 16)
}
// S for one output channel: wc = w_ctx + co * ks * ks, taps added in index order (deterministic)
__device__ __forceinline__ float ctx_tapsum(const float* wc, int taps, unsigned mask) {
  float s = 0.f;
  for (int t = 0; t < taps; ++t) s += ((mask >> t) & 1u) ? wc[t] : 0.f;
  return s;
}
// ... over the 16 taps of ks = 4.  A function of its own for the streamed kernel's 4 x 4 instantiations: beside them, its 5 x 5
// instantiations stay the only callers of ctx_tapsum in their unit, all with 25 taps, and compile to what they did
__device__ __forceinline__ float ctx_tapsum4(const float* wc, unsigned mask) {
  float s = 0.f;
  for (int t = 0; t < 16; ++t) s += ((mask >> t) & 1u) ? wc[t] : 0.f;
  return s;
}

// 64-lane sum via DPP-friendly shuffles (wavefront = 64 on gfx950)
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  return v;
}

}  // namespace usf
