// Small device helpers shared by the GRU recurrence files (csrc/gru.hip, gru16.hip, grumc.hip, gru32.hip).
#pragma once
#include "common.h"

namespace {
constexpr int BG = 16;   // batch rows per recurrence / workgroup of the MFMA kernels (MFMA N)

// time index of processing step s for direction d
__device__ __forceinline__ int t_of(int s, int d, int T) { return d == 0 ? s : T - 1 - s; }

// fast gate nonlinearities of the 16-bit kernels (v_exp_f32 + v_rcp_f32; ~1e-6 relative, well inside the
// bf16-mode budget); the fp32 kernels use b2p_sigmoid / tanhf
__device__ __forceinline__ float sigm(float x) { return __builtin_amdgcn_rcpf(1.f + __expf(-x)); }
__device__ __forceinline__ float tanh_fast(float x) { return 1.f - 2.f * __builtin_amdgcn_rcpf(1.f + __expf(2.f * x)); }

__device__ __forceinline__ bf16x8 pack8_strided(const float* p, int64_t stride) {
  bf16x8 r;
#pragma unroll
  for (int j = 0; j < 8; ++j) r[j] = (__bf16)p[j * stride];
  return r;
}
}  // namespace
