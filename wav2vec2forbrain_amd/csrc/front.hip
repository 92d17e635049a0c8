// The bf16 mode's front end in one pass: GaussianSmoothing -> day linear (+ bias) -> softsign, and the 16-bit
// source image of the implicit-Unfold projection, for C = 256 channels.
//
// Today's three launches (gauss_k, gemm_kernel with gathered weights / bias / pre_out / softsign, cast16_tail_k)
// read or write the (B, L, 256) fp32 tensor seven times. Here a workgroup owns FR = 32 time rows of one sample:
//   1. the rows and their tap halo go from HBM into LDS once (rows outside [0, L) are not loaded: their taps
//      are skipped, not multiplied by zero);
//   2. each thread smooths (row, 4 channels) items from the LDS tile with gauss_k's chain (taps in increasing j
//      from a zero accumulator, acc += w * v), stores xs and puts its 16-bit value into the A-operand tile;
//   3. the four waves multiply the 32 x 256 tile by W[day] (64 columns each): A fragments from LDS, B fragments
//      straight from global memory (W[day] is 256 KB and stays in L2; two steps of loads ahead of the MFMAs, the
//      first pair issued before step 1), converted as gemm_kernel converts its fp32 operands (mfma16.h), eight
//      32-deep MFMAs in increasing k into one accumulator per output element;
//   4. the accumulators get gemm_epi.h's bias add, cross LDS (over the halo tile, which is dead by then) and leave
//      as float4 rows: z, s = z / (1 + |z|), and the 16-bit image of s.
// The last workgroup also writes the image's zero tail. Every output equals the three-launch path's bit for bit.
#include "common.h"
#include "../../include/b2p_hip.h"
#include "mfma16.h"

namespace {

constexpr int FC = 256;          // channels (= K = N of the day linear)
constexpr int FR = 32;           // time rows per workgroup
constexpr int FLS = FC + 8;      // 16-bit A tile row stride: rows 16-B aligned, odd multiple of 16 B
constexpr int FZS = FC + 4;      // fp32 output tile row stride
constexpr int FRONT_MAX_TAPS = 64;

__host__ __device__ constexpr int front_halo_bytes(int ntaps) {
  const int halo = (FR + ntaps - 1) * FC * 4, zt = FR * FZS * 4;
  return halo > zt ? halo : zt;
}
inline int front_lds_bytes(int ntaps) { return front_halo_bytes(ntaps) + FR * FLS * 2; }

template <int PREC>
__global__ void __launch_bounds__(256) front_fwd_k(const float* __restrict__ x, const float* __restrict__ taps,
                                                   int ntaps, const int64_t* __restrict__ day,
                                                   const float* __restrict__ W, const float* __restrict__ bias,
                                                   float* __restrict__ xs, float* __restrict__ z,
                                                   float* __restrict__ s, uint16_t* __restrict__ s16, int s16_half,
                                                   int64_t tail4, int L) {
  extern __shared__ __attribute__((aligned(16))) unsigned char front_smem[];
  float* xh = reinterpret_cast<float*>(front_smem);                                    // [FR + ntaps - 1][FC]
  float* zt = reinterpret_cast<float*>(front_smem);                                    // [FR][FZS], after step 2
  uint16_t* a16 = reinterpret_cast<uint16_t*>(front_smem + front_halo_bytes(ntaps));   // [FR][FLS]

  const int tid = threadIdx.x;
  const int b = blockIdx.y;
  const int l0 = blockIdx.x * FR;
  const int left = (ntaps - 1) / 2;
  const int c4 = tid & 63, rq = tid >> 6;
  const int64_t sample = (int64_t)b * L * FC;

  // W[day] fragments of the first two 32-deep steps: their L2 latency passes behind steps 1 and 2
  const int lane = tid & 63, wave = tid >> 6;
  const int l16 = lane & 15, g = lane >> 4;
  const int64_t d = day[b];
  const float* Wd = W + d * FC * FC;
  Col8 rb[2][2][4];   // [register buffer][step of the pair][column tile]
#pragma unroll
  for (int q = 0; q < 2; ++q)
#pragma unroll
    for (int j = 0; j < 4; ++j) rb[0][q][j] = col_load(Wd, FC, 64 * wave + 16 * j + l16, 32 * q + 8 * g, 0, FC);

  // 1. halo tile
  const int nh = FR + ntaps - 1;
  for (int r0 = rq; r0 < nh; r0 += 64) {   // 16 rows per thread in flight (rows outside load a clamped row)
    float4 v[16];
#pragma unroll
    for (int u = 0; u < 16; ++u) {
      const int src = l0 + r0 + 4 * u - left;
      const int sc = src < 0 ? 0 : (src < L ? src : L - 1);
      v[u] = *reinterpret_cast<const float4*>(x + sample + (int64_t)sc * FC + 4 * c4);
    }
#pragma unroll
    for (int u = 0; u < 16; ++u) {
      const int r = r0 + 4 * u, src = l0 + r - left;
      if (r < nh && src >= 0 && src < L) *reinterpret_cast<float4*>(xh + r * FC + 4 * c4) = v[u];
    }
  }
  __syncthreads();

  // 2. smoothing: the thread's eight rows rq, rq + 4, ... side by side, each row's chain in increasing j
  {
    float4 acc[FR / 4];
#pragma unroll
    for (int u = 0; u < FR / 4; ++u) acc[u] = make_float4(0, 0, 0, 0);
    for (int j = 0; j < ntaps; ++j) {
      const float w = taps[j];
#pragma unroll
      for (int u = 0; u < FR / 4; ++u) {
        const int r = rq + 4 * u;
        const int src = l0 + r + j - left;
        if (src < 0 || src >= L) continue;   // a tap outside the sample (its halo row was not loaded)
        const float4 v = *reinterpret_cast<const float4*>(xh + (r + j) * FC + 4 * c4);
        acc[u].x += w * v.x; acc[u].y += w * v.y; acc[u].z += w * v.z; acc[u].w += w * v.w;
      }
    }
#pragma unroll
    for (int u = 0; u < FR / 4; ++u) {
      const int r = rq + 4 * u, l = l0 + r;
      if (l >= L) acc[u] = make_float4(0, 0, 0, 0);   // rows past the sample: a zero operand row, nothing stored
      else *reinterpret_cast<float4*>(xs + sample + (int64_t)l * FC + 4 * c4) = acc[u];
      *reinterpret_cast<typename Frag<PREC>::V4*>(a16 + r * FLS + 4 * c4) = Frag<PREC>::cvt4(acc[u]);
    }
  }
  __syncthreads();

  // 3. 32 x 256 x 256 product: wave w owns columns 64 w .. 64 w + 63; the next pair of steps is loaded while
  // this pair multiplies
  f32x4 acc[2][4];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int p = 0; p < FC / 64; ++p) {
    if (p + 1 < FC / 64) {
#pragma unroll
      for (int q = 0; q < 2; ++q)
#pragma unroll
        for (int j = 0; j < 4; ++j)
          rb[(p + 1) & 1][q][j] = col_load(Wd, FC, 64 * wave + 16 * j + l16, 64 * (p + 1) + 32 * q + 8 * g, 0, FC);
    }
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      const int ks = 2 * p + q;
      typename Frag<PREC>::V af[2];
#pragma unroll
      for (int i = 0; i < 2; ++i)
        af[i] = *reinterpret_cast<const typename Frag<PREC>::V*>(a16 + (16 * i + l16) * FLS + 32 * ks + 8 * g);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const typename Frag<PREC>::V bf = Frag<PREC>::cvt(rb[p & 1][q][j].x);
#pragma unroll
        for (int i = 0; i < 2; ++i) acc[i][j] = Frag<PREC>::mfma(af[i], bf, acc[i][j]);
      }
    }
  }

  // 4. bias, then through LDS (the halo tile was last read before the barrier above) to row-wide stores
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const int n = 64 * wave + 16 * j + l16;
    const float bv = bias[d * FC + n];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        float v = acc[i][j][r];
        v += bv;
        zt[(16 * i + 4 * g + r) * FZS + n] = v;
      }
  }
  __syncthreads();
#pragma unroll 2
  for (int r = rq; r < FR; r += 4) {
    const int l = l0 + r;
    if (l >= L) break;
    const float4 v = *reinterpret_cast<const float4*>(zt + r * FZS + 4 * c4);
    const int64_t o = sample + (int64_t)l * FC + 4 * c4;
    *reinterpret_cast<float4*>(z + o) = v;
    const float4 a = make_float4(v.x / (1.0f + fabsf(v.x)), v.y / (1.0f + fabsf(v.y)), v.z / (1.0f + fabsf(v.z)),
                                 v.w / (1.0f + fabsf(v.w)));
    *reinterpret_cast<float4*>(s + o) = a;
    if (s16) *reinterpret_cast<uint2*>(s16 + o) = b2p_pack16x4(a, s16_half != 0);
  }
  if (s16 && blockIdx.x == gridDim.x - 1 && blockIdx.y == gridDim.y - 1) {
    uint2* t = reinterpret_cast<uint2*>(s16 + (int64_t)gridDim.y * L * FC);
    for (int64_t i = tid; i < tail4; i += 256) t[i] = make_uint2(0u, 0u);
  }
}

}  // namespace

extern "C" int b2p_front_fwd(const float* x, const float* taps, int ntaps, const int64_t* day, int64_t n_days,
                             const float* W, const float* bias, float* xs, float* z, float* s, uint16_t* s16,
                             int s16_fp16, int64_t s16_tail, int64_t B, int64_t L, int64_t C, int precision,
                             b2p_stream_t stream) {
  B2P_CHECK_ARG(x && taps && day && W && bias && xs && z && s, "front_fwd: NULL pointer");
  B2P_CHECK_ARG(C == FC, "front_fwd: C must be %d (got %lld): use b2p_gauss_smooth, b2p_gemm and b2p_cast16_tail", FC,
                (long long)C);
  B2P_CHECK_ARG(ntaps >= 1 && ntaps <= FRONT_MAX_TAPS, "front_fwd: ntaps must be 1..%d", FRONT_MAX_TAPS);
  B2P_CHECK_ARG(precision == 0 || precision == 2, "front_fwd: precision must be 0 (bf16 MFMA) or 2 (fp16 MFMA)");
  B2P_CHECK_ARG(B >= 0 && L >= 0 && n_days >= 1 && B <= 65535 && L < (1ll << 31) - FR && B * L * C < (1ll << 40),
                "front_fwd: bad shape");
  B2P_CHECK_ARG(s16_tail >= 0 && s16_tail % 4 == 0, "front_fwd: the image's tail must be a multiple of 4");
  for (const void* p : {(const void*)x, (const void*)W, (const void*)bias, (const void*)xs, (const void*)z,
                        (const void*)s})
    B2P_CHECK_ARG(((uintptr_t)p & 15u) == 0, "front_fwd: tensors must be 16-byte aligned");
  B2P_CHECK_ARG(((uintptr_t)s16 & 7u) == 0, "front_fwd: the 16-bit image must be 8-byte aligned");
  // gemm_kernel skips its K loop under a closed LayerDrop gate: the front end never runs under one
  B2P_CHECK_ARG(!b2p_gate() && !b2p_gate_batch(), "front_fwd: a LayerDrop gate is set");
  if (B == 0 || L == 0) return 0;
  const int lds = front_lds_bytes(ntaps);
  static bool attr[2] = {false, false};
  const int h = precision == 2;
  if (!attr[h]) {
    if (h) B2P_CHECK_HIP(hipFuncSetAttribute((const void*)front_fwd_k<2>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                             front_lds_bytes(FRONT_MAX_TAPS)));
    else B2P_CHECK_HIP(hipFuncSetAttribute((const void*)front_fwd_k<0>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                           front_lds_bytes(FRONT_MAX_TAPS)));
    attr[h] = true;
  }
  const dim3 grid((unsigned)((L + FR - 1) / FR), (unsigned)B);
  if (h)
    hipLaunchKernelGGL(front_fwd_k<2>, grid, dim3(256), lds, (hipStream_t)stream, x, taps, ntaps, day, W, bias, xs, z, s,
                       s16, s16_fp16, s16_tail / 4, (int)L);
  else
    hipLaunchKernelGGL(front_fwd_k<0>, grid, dim3(256), lds, (hipStream_t)stream, x, taps, ntaps, day, W, bias, xs, z, s,
                       s16, s16_fp16, s16_tail / 4, (int)L);
  B2P_CHECK_LAUNCH();
  return 0;
}
