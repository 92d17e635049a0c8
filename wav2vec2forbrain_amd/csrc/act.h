// The activation table of the elementwise kernels b2p_act_fwd / b2p_act_bwd (elementwise.hip):
// value and derivative of every B2P_ACT_* id, the id a template parameter (the host switches once
// per launch). Ids 0-3 are the expressions the GEMM epilogues fuse (gemm_epi.h), unchanged; the
// others follow transformers' activations.py and exist only here: a Linear with one of them runs
// as GEMM (bias, pre-activation out) + b2p_act_fwd.
//
// Every form is finite for every finite fp32 input whose true result is: exponentials are taken
// of -|z| only, 1 - s and 1 - t*t are never formed by subtraction, and a product 0 * inf cannot
// arise (a saturated factor is selected away, not multiplied). Library expf / tanhf / erfcf, not
// the fast forms: these kernels move 8-12 bytes per element.
#pragma once
#include "common.h"
#include "../../include/b2p_hip.h"

// sigmoid(z) and sigmoid'(z) = s (1 - s) from one exponential of -|z|
__device__ __forceinline__ void b2p_sig_parts(float z, float& s, float& ds) {
  const float e = expf(-fabsf(z));
  const float r = 1.0f / (1.0f + e);
  s = z >= 0.0f ? r : e * r;
  ds = e * r * r;
}
// 2 u(x) of the tanh GELU, 0.5 x (1 + tanh u) = x sigmoid(2 u), u = sqrt(2/pi) (x + 0.044715 x^3)
__device__ __forceinline__ float b2p_gelu_tanh_2u(float x) {
  return 1.5957691216057308f * (x + 0.044715f * (x * x * x));
}
// Phi(x) = 0.5 erfc(-x / sqrt 2): relative accuracy in the negative tail
__device__ __forceinline__ float b2p_phi_erfc(float x) { return 0.5f * erfcf(-0.70710678118654752440f * x); }
// Mish: t = tanh(softplus(x)), omt = 1 - t, s = sigmoid(x), from e = exp(-|x|).
// With w = e^x, tanh(log(1 + w)) = w (w + 2) / (w (w + 2) + 2); for x > 0 the same scaled by e^-2x.
__device__ __forceinline__ void b2p_mish_parts(float x, float& t, float& omt, float& s) {
  const float e = expf(-fabsf(x));
  const float r = 1.0f / (1.0f + e);
  if (x > 0.0f) {
    const float num = fmaf(2.0f, e, 1.0f), k = 2.0f * e * e, inv = 1.0f / (num + k);
    t = num * inv; omt = k * inv; s = r;
  } else {
    const float num = e * (e + 2.0f), inv = 1.0f / (num + 2.0f);
    t = num * inv; omt = 2.0f * inv; s = e * r;
  }
}

template <int ACT> __device__ __forceinline__ float b2p_act_val(float x) {
  if constexpr (ACT == B2P_ACT_GELU) return b2p_gelu(x);
  else if constexpr (ACT == B2P_ACT_SOFTSIGN) return x / (1.0f + fabsf(x));
  else if constexpr (ACT == B2P_ACT_SILU) return b2p_silu(x);
  else if constexpr (ACT == B2P_ACT_GELU_TANH) {
    float s, ds;
    b2p_sig_parts(b2p_gelu_tanh_2u(x), s, ds);
    return x * s;
  } else if constexpr (ACT == B2P_ACT_GELU_10) return fminf(x * b2p_phi_erfc(x), 10.0f);   // gelu >= -0.17
  else if constexpr (ACT == B2P_ACT_QUICK_GELU) {
    float s, ds;
    b2p_sig_parts(1.702f * x, s, ds);
    return x * s;
  } else if constexpr (ACT == B2P_ACT_LAPLACE)
    return 0.5f * erfcf((0.707107f - x) * 2.506626424383798f);   // 1 / (0.282095 sqrt 2)
  else if constexpr (ACT == B2P_ACT_MISH) {
    float t, omt, s;
    b2p_mish_parts(x, t, omt, s);
    return x * t;
  } else if constexpr (ACT == B2P_ACT_RELU) return fmaxf(x, 0.0f);
  else if constexpr (ACT == B2P_ACT_RELU2) { const float r = fmaxf(x, 0.0f); return r * r; }
  else if constexpr (ACT == B2P_ACT_RELU6) return fminf(fmaxf(x, 0.0f), 6.0f);
  else if constexpr (ACT == B2P_ACT_SIGMOID) {
    float s, ds;
    b2p_sig_parts(x, s, ds);
    return s;
  } else if constexpr (ACT == B2P_ACT_TANH) return tanhf(x);
  else return x;
}

template <int ACT> __device__ __forceinline__ float b2p_act_grad(float x) {
  if constexpr (ACT == B2P_ACT_GELU) return b2p_gelu_grad(x);
  else if constexpr (ACT == B2P_ACT_SOFTSIGN) { const float d = 1.f + fabsf(x); return 1.f / (d * d); }
  else if constexpr (ACT == B2P_ACT_SILU) return b2p_silu_grad(x);
  else if constexpr (ACT == B2P_ACT_GELU_TANH) {
    // s + x s (1 - s) (2u)'; beyond |x| = 10 (|2u| > 87) the second term is below 1e-35 and its
    // factors are 0 and a square that overflows
    float s, ds;
    b2p_sig_parts(b2p_gelu_tanh_2u(x), s, ds);
    const float du = 1.5957691216057308f * fmaf(0.134145f, x * x, 1.0f);
    return fabsf(x) > 10.0f ? s : fmaf(x * ds, du, s);
  } else if constexpr (ACT == B2P_ACT_GELU_10) {
    // Phi(x) + x phi(x); 0 where the clip is active (x Phi(x) > 10 <=> x > 10 in fp32)
    const float cdf = b2p_phi_erfc(x);
    const float pdf = 0.39894228040143267794f * expf(-0.5f * (x * x));
    return x * cdf > 10.0f ? 0.0f : fmaf(x, pdf, cdf);
  } else if constexpr (ACT == B2P_ACT_QUICK_GELU) {
    float s, ds;
    b2p_sig_parts(1.702f * x, s, ds);
    return fmaf(1.702f, x * ds, s);
  } else if constexpr (ACT == B2P_ACT_LAPLACE) {
    const float z = (x - 0.707107f) * 2.506626424383798f;
    return 1.4142125184828966f * expf(-(z * z));   // 1 / (0.282095 sqrt(2 pi))
  } else if constexpr (ACT == B2P_ACT_MISH) {
    // t + x (1 - t^2) sigmoid(x), 1 - t^2 = (1 - t)(1 + t)
    float t, omt, s;
    b2p_mish_parts(x, t, omt, s);
    return fmaf(x * s, omt * (1.0f + t), t);
  } else if constexpr (ACT == B2P_ACT_RELU) return x > 0.0f ? 1.0f : 0.0f;
  else if constexpr (ACT == B2P_ACT_RELU2) return 2.0f * fmaxf(x, 0.0f);
  else if constexpr (ACT == B2P_ACT_RELU6) return x > 0.0f && x < 6.0f ? 1.0f : 0.0f;
  else if constexpr (ACT == B2P_ACT_SIGMOID) {
    float s, ds;
    b2p_sig_parts(x, s, ds);
    return ds;
  } else if constexpr (ACT == B2P_ACT_TANH) {
    // 1 - tanh^2 x = 4 sigmoid'(2x)
    float s, ds;
    b2p_sig_parts(2.0f * x, s, ds);
    return 4.0f * ds;
  } else return 1.0f;
}
