// Adam / AdamW and clip_grad_norm_ over ALL parameter tensors of a parameter group: tables of chunks, one 256-thread block
// per chunk, as the SophiaG kernels (usf_train.hip).  See include/usflows_hip_internal.h for the contracts.
#include <math.h>

#include "usf_common.h"

namespace usf {

// ---------------------------------------------------------------------------------------------------------
// Adam (torch/optim/adam.py, _single_tensor_adam, the non-capturable branch), its operation order in fp32:
//   g' = maximize ? -g : g;   L2: g' = fma(wd, p, g')   |   decoupled (AdamW): p *= 1 - lr * wd
//   m  = lerp(m, g', 1 - beta1)            (ATen: |w| < 0.5 ? fma(w, g' - m, m) : fma(g' - m, w - 1, g'))
//   v  = v * beta2 + ((1 - beta2) * g') * g';   amsgrad: vmax = max(vmax, v)
//   denom = sqrt(v | vmax) / sqrt(1 - beta2^t) + eps;   p += (-lr / (1 - beta1^t)) * (m / denom)
// t is the DEVICE step counter steps[slot], advanced by adam_advance_kernel in a launch of its own before this one: the
// value lives in memory, so a hipGraph replay of the pair computes with the step it is at, not the one it was captured
// at.  beta^t in fp64, once per block (thread 0, broadcast through LDS).  28 bytes per parameter and step (36: amsgrad).
// ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void adam_advance_kernel(int64_t* __restrict__ steps, int n_slots) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n_slots) steps[i] += 1;
}

struct AdamArgs {
  double lr, beta1, beta2;
  float decay;      // 1 - lr * wd (decoupled), else unused
  float wd;         // L2 coefficient (0: none)
  float w1;         // 1 - beta1: the lerp weight
  float beta2f, omb2, eps;
  int32_t maximize, amsgrad, decoupled;
};

__global__ __launch_bounds__(256) void adam_step_kernel(const usf_adam_chunk* __restrict__ chunks,
                                                        const int64_t* __restrict__ steps, AdamArgs a) {
  __shared__ float s_corr[2];
  const usf_adam_chunk c = chunks[blockIdx.x];
  if (threadIdx.x == 0) {
    const double t = (double)steps[c.slot];
    const double bc1 = 1.0 - pow(a.beta1, t), bc2 = 1.0 - pow(a.beta2, t);
    s_corr[0] = (float)(-(a.lr / bc1));     // value of addcdiv_: -step_size, rounded to fp32 once
    s_corr[1] = (float)sqrt(bc2);           // bias_correction2 ** 0.5
  }
  __syncthreads();
  const float neg_step = s_corr[0], bc2_sqrt = s_corr[1];
  const bool low = fabsf(a.w1) < 0.5f;
  const float w1m1 = a.w1 - 1.f;
  for (int i = threadIdx.x; i < c.n; i += 256) {
    float g = c.g[i];
    if (a.maximize) g = -g;
    float p = c.p[i];
    if (a.wd != 0.f) {
      if (a.decoupled) p *= a.decay;
      else g = fmaf(a.wd, p, g);
    }
    const float m0 = c.m[i];
    const float d = g - m0;
    const float m = low ? fmaf(a.w1, d, m0) : fmaf(d, w1m1, g);
    float v = c.v[i] * a.beta2f + (a.omb2 * g) * g;
    c.m[i] = m;
    c.v[i] = v;
    if (a.amsgrad) {
      const float vm = c.vmax[i];
      v = (vm > v || vm != vm) ? vm : v;    // torch.maximum: a NaN on either side stays
      c.vmax[i] = v;
    }
    const float denom = sqrtf(v) / bc2_sqrt + a.eps;
    c.p[i] = p + neg_step * (m / denom);
  }
}

int adam_step(const usf_adam_chunk* chunks, int64_t n_chunks, int64_t* steps, int64_t n_slots, double lr, double beta1,
              double beta2, double eps, double weight_decay, int32_t flags, hipStream_t stream) {
  if (n_chunks < 0 || n_chunks > 0x7fffffff || n_slots < 0 || n_slots > 0x7fffffff || (n_chunks > 0 && (!chunks || !steps || n_slots == 0)) ||
      (flags & ~7)) {
    set_error("usf_adam_step_f32: bad arguments");
    return -1;
  }
  if (n_chunks == 0) return 0;
  AdamArgs a;
  a.lr = lr; a.beta1 = beta1; a.beta2 = beta2;
  a.maximize = flags & 1; a.amsgrad = (flags >> 1) & 1; a.decoupled = (flags >> 2) & 1;
  a.decay = (float)(1.0 - lr * weight_decay);
  a.wd = (float)weight_decay;
  a.w1 = (float)(1.0 - beta1);
  a.beta2f = (float)beta2;
  a.omb2 = (float)(1.0 - beta2);
  a.eps = (float)eps;
  adam_advance_kernel<<<(unsigned)((n_slots + 255) / 256), 256, 0, stream>>>(steps, (int)n_slots);
  int rc = check_launch("usf_adam_step_f32 (advance)");
  if (rc) return rc;
  adam_step_kernel<<<(unsigned)n_chunks, 256, 0, stream>>>(chunks, steps, a);
  return check_launch("usf_adam_step_f32");
}

// ---------------------------------------------------------------------------------------------------------
// torch.nn.utils.clip_grad_norm_(params, max_norm) (norm 2, error_if_nonfinite=False) in two launches, no atomics:
//   1. partials[b] = sum of squares of chunk b in fp64 (squares of fp32 values are exact there), reduced in a fixed order:
//      thread t sums elements t, t + 256, ... ascending, then a fixed LDS tree.
//   2. every block adds ALL partials in the same fixed order (so all blocks hold the same total bit for bit), forms
//      coef = min(max_norm / (sqrt(total) + 1e-6), 1) in fp64, rounds it to fp32 ONCE and scales its own chunk in place.
// A NaN / inf norm propagates as in torch (coef NaN -> NaN gradients; inf -> coef 0).
// ---------------------------------------------------------------------------------------------------------
__device__ __forceinline__ double block_sum_256(double v, double* lds) {
  lds[threadIdx.x] = v;
  __syncthreads();
#pragma unroll
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) lds[threadIdx.x] += lds[threadIdx.x + o];
    __syncthreads();
  }
  const double r = lds[0];
  __syncthreads();
  return r;
}

__global__ __launch_bounds__(256) void grad_sqnorm_partials_kernel(const usf_grad_chunk* __restrict__ chunks,
                                                                   double* __restrict__ partials) {
  __shared__ double lds[256];
  const usf_grad_chunk c = chunks[blockIdx.x];
  double s = 0.0;
  for (int i = threadIdx.x; i < c.n; i += 256) {
    const double g = (double)c.g[i];
    s += g * g;
  }
  s = block_sum_256(s, lds);
  if (threadIdx.x == 0) partials[blockIdx.x] = s;
}

__global__ __launch_bounds__(256) void grad_clip_scale_kernel(const usf_grad_chunk* __restrict__ chunks,
                                                              const double* __restrict__ partials, int n_chunks, double max_norm) {
  __shared__ double lds[256];
  double s = 0.0;
  for (int i = threadIdx.x; i < n_chunks; i += 256) s += partials[i];
  const double total = block_sum_256(s, lds);
  const double coef = max_norm / (sqrt(total) + 1e-6);
  const float clamped = coef > 1.0 ? 1.f : (float)coef;      // (torch.clamp(max=1.0): a NaN stays a NaN)
  const usf_grad_chunk c = chunks[blockIdx.x];
  for (int i = threadIdx.x; i < c.n; i += 256) c.g[i] *= clamped;
}

int grad_sqnorm_partials(const usf_grad_chunk* chunks, int64_t n_chunks, double* partials, hipStream_t stream) {
  if (n_chunks < 0 || n_chunks > 0x7fffffff || (n_chunks > 0 && (!chunks || !partials))) {
    set_error("usf_grad_sqnorm_partials_f32: bad arguments");
    return -1;
  }
  if (n_chunks == 0) return 0;
  grad_sqnorm_partials_kernel<<<(unsigned)n_chunks, 256, 0, stream>>>(chunks, partials);
  return check_launch("usf_grad_sqnorm_partials_f32");
}

int grad_clip_scale(const usf_grad_chunk* chunks, int64_t n_chunks, const double* partials, double max_norm, hipStream_t stream) {
  if (n_chunks < 0 || n_chunks > 0x7fffffff || (n_chunks > 0 && (!chunks || !partials))) {
    set_error("usf_grad_clip_scale_f32: bad arguments");
    return -1;
  }
  if (n_chunks == 0) return 0;
  grad_clip_scale_kernel<<<(unsigned)n_chunks, 256, 0, stream>>>(chunks, partials, (int)n_chunks, max_norm);
  return check_launch("usf_grad_clip_scale_f32");
}

}  // namespace usf
