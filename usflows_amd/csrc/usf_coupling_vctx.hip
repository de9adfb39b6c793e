// The vector-context instantiations of the three fused additive-coupling kernels (usf_coupling_additive_vctx_f32,
// include/usflows_hip_internal.h): each kernel file compiled a second time with USF_VCTX defined -- its kernel under the _vctx
// name with the rank-ctx_dim context step (vctx_add, usf_common.h; the tiny-layer kernel: LDS-resident segments), and the launch
// function its dispatcher calls.  A translation unit of its own: the files' own objects hold the kernels without a vector
// context exactly as they were.
#define USF_VCTX 1
#include "usf_coupling.hip"
#include "usf_coupling_bf16x3.hip"
#include "usf_coupling_tiny.hip"
