// Skinny GEMMs of a 32-wide head (the CTC lm_head: 7968 x 32 x 768) on fp32 operands in HBM.
//
// gemm_kernel (gemm.hip) gives such a product 128-row tiles: 63 workgroups on 256 CUs, three quarters of
// every tile empty. The three kernels here shape the same arithmetic to the problem: every wave loads its
// MFMA fragments straight from global memory (no LDS, no barrier), converts them as gemm_kernel does while
// staging (bf16 by plain cast, precision 0; saturated fp16, precision 2) and feeds the same instruction
// (v_mfma_f32_16x16x32_bf16 / _f16) with the same k of every lane: lane holds row / column (lane & 15) and
// k = 32*step + 8*(lane >> 4) .. +7. Every output element keeps one accumulator that starts at zero and
// takes its MFMAs in increasing k, so the results equal gemm_kernel's bit for bit (k past the end is
// zero in both; gemm_kernel's MFMAs on all-zero fragments add +0 to an accumulator that is never -0).
//   forward        C[M][32]  = A[M][K] . W[32][K]^T (+ bias)     16 rows per wave, 2 waves per workgroup
//   backward-data  dA[M][N]  = dC[M][32] . W[32][N]              32 rows per workgroup, column tiles over 4 waves
//   weight grad.   dW[32][N] = dC[Kt][32]^T . X[Kt][N]           one 16 x 16 tile per wave, K slices as the
//                  descriptor's ksplit / kchunk say, slabs summed by splitk_reduce4 as after gemm_kernel
#include "common.h"
#include "../../include/b2p_hip.h"
#include "timing.h"
#include "gemm_epi.h"
#include "mfma16.h"

namespace {

// Every kernel issues the loads of UN 32-deep steps (or column tiles) before it converts and multiplies any of
// them, so a wave keeps UN steps of memory traffic in flight with no LDS stage behind it. Steps past the end of
// K are all-zero fragments (MFMAs that add +0).
constexpr int UN = 4;

// ------------------------------------------------------------------ forward
template <int PREC>
__global__ void __launch_bounds__(128) skinny32_fwd_k(const float* __restrict__ A, int64_t lda,
                                                      const float* __restrict__ W, int64_t ldw,
                                                      const float* __restrict__ bias, float* __restrict__ C,
                                                      int64_t ldc, int M, int K) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int l16 = lane & 15, g = lane >> 4;
  const int m0 = (blockIdx.x * 2 + wave) * 16;
  if (m0 >= M) return;
  const int mr = m0 + l16 < M ? m0 + l16 : M - 1;   // rows past the end read the last row, are not stored
  const float* a = A + (int64_t)mr * lda;
  const float* w0 = W + (int64_t)l16 * ldw;
  const float* w1 = W + (int64_t)(16 + l16) * ldw;
  f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
  for (int k0 = 0; k0 < K; k0 += 32 * UN) {
    Row8 ra[UN], r0[UN], r1[UN];
#pragma unroll
    for (int u = 0; u < UN; ++u) {
      const int k = k0 + 32 * u + 8 * g;
      ra[u] = row_load(a, k, K);
      r0[u] = row_load(w0, k, K);
      r1[u] = row_load(w1, k, K);
    }
#pragma unroll
    for (int u = 0; u < UN; ++u) {
      const typename Frag<PREC>::V af = row_cvt<PREC>(ra[u]);
      acc0 = Frag<PREC>::mfma(af, row_cvt<PREC>(r0[u]), acc0);
      acc1 = Frag<PREC>::mfma(af, row_cvt<PREC>(r1[u]), acc1);
    }
  }
  const float bv0 = bias ? bias[l16] : 0.f, bv1 = bias ? bias[16 + l16] : 0.f;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int m = m0 + 4 * g + r;
    if (m >= M) continue;
    float v0 = acc0[r], v1 = acc1[r];
    if (bias) { v0 += bv0; v1 += bv1; }
    C[(int64_t)m * ldc + l16] = v0;
    C[(int64_t)m * ldc + 16 + l16] = v1;
  }
}

// ------------------------------------------------------------------ backward-data (K = 32: one MFMA per tile)
template <int PREC>
__global__ void __launch_bounds__(256) skinny32_dgrad_k(const float* __restrict__ dC, int64_t lddc,
                                                        const float* __restrict__ W, int64_t ldw,
                                                        float* __restrict__ dA, int64_t ldda, int M, int N) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int l16 = lane & 15, g = lane >> 4;
  const int m0 = blockIdx.x * 32;
  typename Frag<PREC>::V af[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int m = m0 + 16 * i + l16;
    af[i] = row_cvt<PREC>(row_load(dC + (int64_t)(m < M ? m : M - 1) * lddc, 8 * g, 32));
  }
  const int ntiles = (N + 15) / 16;
  for (int t0 = wave; t0 < ntiles; t0 += 4 * UN) {   // column tiles wave, wave + 4, ...
    Col8 rb[UN];
#pragma unroll
    for (int u = 0; u < UN; ++u) {
      const int n = 16 * (t0 + 4 * u) + l16;
      rb[u] = col_load(W, ldw, n < N ? n : N - 1, 8 * g, 0, 32);
    }
#pragma unroll
    for (int u = 0; u < UN; ++u) {
      const int n = 16 * (t0 + 4 * u) + l16;
      const typename Frag<PREC>::V bf = Frag<PREC>::cvt(rb[u].x);
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const f32x4 acc = Frag<PREC>::mfma(af[i], bf, f32x4{0.f, 0.f, 0.f, 0.f});
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int m = m0 + 16 * i + 4 * g + r;
          if (m < M && n < N) dA[(int64_t)m * ldda + n] = acc[r];
        }
      }
    }
  }
}

// ------------------------------------------------------------------ weight gradient
// grid (ceil(N / 32), K slices); wave: row tile wave & 1, column tile 2*blockIdx.x + (wave >> 1).
// out = the slice's slab (ld N) under split-K, else the result itself.
template <int PREC>
__global__ void __launch_bounds__(256) skinny32_wgrad_k(const float* __restrict__ dC, int64_t lddc,
                                                        const float* __restrict__ X, int64_t ldx,
                                                        float* __restrict__ out, int64_t ldo, int64_t slab, int N,
                                                        int K, int kchunk) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int l16 = lane & 15, g = lane >> 4;
  const int mt = wave & 1, nt = 2 * blockIdx.x + (wave >> 1);
  if (16 * nt >= N) return;
  const int kbeg = blockIdx.y * kchunk;
  const int kend = K < kbeg + kchunk ? K : kbeg + kchunk;
  const int n = 16 * nt + l16;
  const int nc = n < N ? n : N - 1;
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  for (int k0 = kbeg; k0 < kend; k0 += 32 * UN) {
    Col8 ra[UN], rb[UN];
#pragma unroll
    for (int u = 0; u < UN; ++u) {
      ra[u] = col_load(dC, lddc, 16 * mt + l16, k0 + 32 * u + 8 * g, kbeg, kend);
      rb[u] = col_load(X, ldx, nc, k0 + 32 * u + 8 * g, kbeg, kend);
    }
#pragma unroll
    for (int u = 0; u < UN; ++u) acc = Frag<PREC>::mfma(Frag<PREC>::cvt(ra[u].x), Frag<PREC>::cvt(rb[u].x), acc);
  }
  float* o = out + (int64_t)blockIdx.y * slab;
  if (n < N) {
#pragma unroll
    for (int r = 0; r < 4; ++r) o[(int64_t)(16 * mt + 4 * g + r) * ldo + n] = acc[r];
  }
}

bool al16(const void* p) { return ((uintptr_t)p & 15u) == 0; }

bool plain_operand(const b2p_operand& o) {
  return o.ptr && o.dtype == 0 && !o.conv && !o.gather1 && al16(o.ptr) && o.ld % 4 == 0;
}

}  // namespace

extern "C" int b2p_skinny32_form(const b2p_gemm_desc* dp) {
  if (!dp) return B2P_SKINNY32_NONE;
  const b2p_gemm_desc& d = *dp;
  const b2p_epilogue& e = d.ep;
  if (d.precision != 0 && d.precision != 2) return B2P_SKINNY32_NONE;
  if (d.nz1 != 1 || d.nz2 != 1 || !plain_operand(d.A) || !plain_operand(d.B)) return B2P_SKINNY32_NONE;
  if (d.M < 1 || d.N < 1 || d.K < 1 || d.M >= (1ll << 31) || d.N >= (1ll << 31) || d.K >= (1ll << 31))
    return B2P_SKINNY32_NONE;
  if (!e.C || e.C16 || e.alpha != 1.f || e.beta != 0.f || e.bias_gather || e.pre_out || e.pre16 || e.aux || e.aux16 ||
      e.act != B2P_ACT_NONE || e.act_bwd != B2P_ACT_NONE || e.drop_p != 0.f || e.residual || e.colsum_part || e.C16b ||
      e.ldc < d.N)
    return B2P_SKINNY32_NONE;
  // a LayerDrop gate skips gemm_kernel's K loop: such a launch stays there
  if (b2p_gate() || b2p_gate_batch()) return B2P_SKINNY32_NONE;
  const bool ak = d.A.inner_is_k != 0, bk = d.B.inner_is_k != 0;
  if (ak && bk && d.N == 32 && d.K % 4 == 0 && d.ksplit <= 1 && d.A.ld >= d.K && d.B.ld >= d.K)
    return B2P_SKINNY32_FWD;
  if (e.bias) return B2P_SKINNY32_NONE;
  if (ak && !bk && d.K == 32 && d.ksplit <= 1 && d.A.ld >= 32 && d.B.ld >= d.N) return B2P_SKINNY32_DGRAD;
  if (!ak && !bk && d.M == 32 && d.A.ld >= 32 && d.B.ld >= d.N) {
    if (d.ksplit > 1 && !(d.workspace && d.kchunk > 0 && d.kchunk % 32 == 0 && (int64_t)d.kchunk * d.ksplit >= d.K &&
                          d.workspace_floats >= (int64_t)d.ksplit * d.M * d.N))
      return B2P_SKINNY32_NONE;
    return B2P_SKINNY32_WGRAD;
  }
  return B2P_SKINNY32_NONE;
}

extern "C" int b2p_skinny32(const b2p_gemm_desc* dp, b2p_stream_t stream) {
  B2P_CHECK_ARG(dp != nullptr, "skinny32: NULL descriptor");
  const int form = b2p_skinny32_form(dp);
  B2P_CHECK_ARG(form != B2P_SKINNY32_NONE,
                "skinny32: not a plain fp32-operand product with a 32-wide side at precision 0 or 2 "
                "(b2p_skinny32_form); use b2p_gemm");
  const b2p_gemm_desc& d = *dp;
  const b2p_epilogue& e = d.ep;
  hipStream_t st = (hipStream_t)stream;
  const float* A = static_cast<const float*>(d.A.ptr);
  const float* B = static_cast<const float*>(d.B.ptr);
  const int M = (int)d.M, N = (int)d.N, K = (int)d.K;
  const bool h = d.precision == 2;
  b2p_timing_begin(d.timing_family, st);
  if (form == B2P_SKINNY32_FWD) {
    const dim3 grid((unsigned)((M + 31) / 32));
    if (h) hipLaunchKernelGGL(skinny32_fwd_k<2>, grid, dim3(128), 0, st, A, d.A.ld, B, d.B.ld, e.bias, e.C, e.ldc, M, K);
    else hipLaunchKernelGGL(skinny32_fwd_k<0>, grid, dim3(128), 0, st, A, d.A.ld, B, d.B.ld, e.bias, e.C, e.ldc, M, K);
  } else if (form == B2P_SKINNY32_DGRAD) {
    const dim3 grid((unsigned)((M + 31) / 32));
    if (h) hipLaunchKernelGGL(skinny32_dgrad_k<2>, grid, dim3(256), 0, st, A, d.A.ld, B, d.B.ld, e.C, e.ldc, M, N);
    else hipLaunchKernelGGL(skinny32_dgrad_k<0>, grid, dim3(256), 0, st, A, d.A.ld, B, d.B.ld, e.C, e.ldc, M, N);
  } else {
    const int ks = d.ksplit > 1 ? d.ksplit : 1;
    const int kchunk = ks > 1 ? d.kchunk : K;
    float* out = ks > 1 ? d.workspace : e.C;
    const int64_t ldo = ks > 1 ? (int64_t)N : e.ldc;
    const dim3 grid((unsigned)((N + 31) / 32), (unsigned)ks);
    if (h)
      hipLaunchKernelGGL(skinny32_wgrad_k<2>, grid, dim3(256), 0, st, A, d.A.ld, B, d.B.ld, out, ldo, (int64_t)M * N,
                         N, K, kchunk);
    else
      hipLaunchKernelGGL(skinny32_wgrad_k<0>, grid, dim3(256), 0, st, A, d.A.ld, B, d.B.ld, out, ldo, (int64_t)M * N,
                         N, K, kchunk);
    if (ks > 1) {   // the slabs are summed as after gemm_kernel (gemm.hip)
      const int64_t total = (int64_t)M * N;
      const bool v4 = N % 4 == 0 && e.ldc % 4 == 0 && al16(e.C) && al16(d.workspace);
      if (v4)
        hipLaunchKernelGGL(splitk_reduce4, dim3((unsigned)((total / 4 + 255) / 256)), dim3(256), 0, st, d.workspace, ks,
                           d.M, d.N, 1, d.ep, total / 4);
      else
        hipLaunchKernelGGL(splitk_reduce, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, d.workspace, ks, d.M,
                           d.N, 1, d.ep, total);
    }
  }
  B2P_CHECK_LAUNCH();
  b2p_timing_end(d.timing_family, st, d.flops);
  return 0;
}
