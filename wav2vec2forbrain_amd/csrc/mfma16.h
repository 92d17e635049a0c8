// 16-bit MFMA fragments built from fp32 values the way gemm_kernel (gemm.hip) stages its fp32 operands:
// precision 0 = bf16 by plain cast on v_mfma_f32_16x16x32_bf16, precision 2 = saturated fp16 on
// v_mfma_f32_16x16x32_f16. Lane l holds row / column l & 15 and k = 8*(l >> 4) .. +7 of a 32-deep step.
#pragma once
#include "common.h"

namespace {

typedef _Float16 h16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 h16x4 __attribute__((ext_vector_type(4)));

template <int PREC> struct Frag;
template <> struct Frag<0> {
  typedef bf16x8 V;
  typedef bf16x4 V4;
  __device__ __forceinline__ static V cvt(const float (&x)[8]) {
    return V{(__bf16)x[0], (__bf16)x[1], (__bf16)x[2], (__bf16)x[3], (__bf16)x[4], (__bf16)x[5], (__bf16)x[6],
             (__bf16)x[7]};
  }
  __device__ __forceinline__ static V4 cvt4(float4 x) { return V4{(__bf16)x.x, (__bf16)x.y, (__bf16)x.z, (__bf16)x.w}; }
  __device__ __forceinline__ static f32x4 mfma(V a, V b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
  }
};
template <> struct Frag<2> {
  typedef h16x8 V;
  typedef h16x4 V4;
  __device__ __forceinline__ static V cvt(const float (&x)[8]) {
    return V{(_Float16)b2p_f16_sat(x[0]), (_Float16)b2p_f16_sat(x[1]), (_Float16)b2p_f16_sat(x[2]),
             (_Float16)b2p_f16_sat(x[3]), (_Float16)b2p_f16_sat(x[4]), (_Float16)b2p_f16_sat(x[5]),
             (_Float16)b2p_f16_sat(x[6]), (_Float16)b2p_f16_sat(x[7])};
  }
  __device__ __forceinline__ static V4 cvt4(float4 x) {
    return V4{(_Float16)b2p_f16_sat(x.x), (_Float16)b2p_f16_sat(x.y), (_Float16)b2p_f16_sat(x.z),
              (_Float16)b2p_f16_sat(x.w)};
  }
  __device__ __forceinline__ static f32x4 mfma(V a, V b, f32x4 c) {
    return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0);
  }
};

// 8 consecutive k of one k-contiguous row (k % 4 == 0, K % 4 == 0: a float4 is inside the row or past it),
// loaded (lanes past the end load the row's first float4) and then converted (those lanes select zero)
struct Row8 {
  float4 a, b;
  bool ok0, ok1;
};
__device__ __forceinline__ Row8 row_load(const float* row, int k, int K) {
  Row8 r;
  r.ok0 = k < K;
  r.ok1 = k + 4 < K;
  r.a = *reinterpret_cast<const float4*>(row + (r.ok0 ? k : 0));
  r.b = *reinterpret_cast<const float4*>(row + (r.ok1 ? k + 4 : 0));
  return r;
}
template <int PREC>
__device__ __forceinline__ typename Frag<PREC>::V row_cvt(const Row8& r) {
  const float x[8] = {r.ok0 ? r.a.x : 0.f, r.ok0 ? r.a.y : 0.f, r.ok0 ? r.a.z : 0.f, r.ok0 ? r.a.w : 0.f,
                      r.ok1 ? r.b.x : 0.f, r.ok1 ? r.b.y : 0.f, r.ok1 ? r.b.z : 0.f, r.ok1 ? r.b.w : 0.f};
  return Frag<PREC>::cvt(x);
}

// 8 consecutive k of one column of a k-major matrix (element (k, c) at p[k*ld + c]); k >= kend reads row
// klo (inside the matrix) and selects zero
struct Col8 {
  float x[8];
};
__device__ __forceinline__ Col8 col_load(const float* p, int64_t ld, int c, int k, int klo, int kend) {
  Col8 r;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const bool ok = k + i < kend;
    const float v = p[(int64_t)(ok ? k + i : klo) * ld + c];
    r.x[i] = ok ? v : 0.f;
  }
  return r;
}

}  // namespace
