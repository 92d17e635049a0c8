// Fused exact-fp32 self-attention (forward + backward) for the w2v / Conformer encoder layers where the
// operands are fp32 (the bf16x3 precision mode by default, the fp32 mode on request: functional.ATTN32_MODES): softmax(Q K^T * scale) -> dropout -> @ V, no mask (reference: eager_attention_forward
// behind HF Wav2Vec2Attention; the Conformer's rotary self-attention core,
// w2v_conformer_custom_feat_extractor.py:79-112). Every product runs on v_mfma_f32_16x16x4_f32 (fp32 operands,
// fp32 accumulate: bitwise an fmaf chain), so nothing is rounded to 16 bits anywhere.
//
// Head size 64 and T' <= 256: one (batch, head)'s K and V as fp32 images are 2 x 64 KB of LDS, so no online
// softmax is needed and the scores never touch HBM (the unfused path runs 6 batched GEMMs and 2 softmax
// kernels per layer over (B, heads, T', T') fp32 tensors and saves two of them for the backward). The work
// split is csrc/attn16.hip's:
//   fwd   (b, h, 128-query block): S^T = K Q^T (keys in registers, query on the lane), in-register softmax,
//         O^T = V^T P^T. Saves lse2[b][h][q] = max + log2(sum) in the log2 domain.
//   dQ    (b, h, 128-query block, launched first): S^T, dP^T recomputed from lse2 and normalised by their own
//         row sum; delta = sum_key P_d dP_d from those same values; both row constants go to delta_ws
//         ([2][B][nh][T]: delta, 1 / row sum); dQ^T += K^T dS^T.
//   dK/dV (b, h, 128-key block): S, dP = dO V^T with the key on the lane; dV^T += dO^T P_d and
//         dK^T += Q^T dS with the dQ pass's delta.
// 257 <= T' <= 512 is the long class further down (attn32_long_*): the same three kernels over two staged
// 256-row chunks, the forward with an online softmax, dQ in two sweeps.
// Fragments. The 16x16x4 operands are one fp32 per lane: A[row = lane & 15][k = lane >> 4] and
// B[k = lane >> 4][col = lane & 15]; C/D register i of lane (g = lane >> 4, lr = lane & 15) is row 4g + i,
// column lr. The order of k inside a sum is free as long as A and B agree, so
//   - a product over the head dimension takes d = 16g + s in step s (s < 16): a lane's 16 operands are 64
//     contiguous bytes of its row (four 16-byte reads from LDS or global memory);
//   - a product over keys (or queries) takes the score tile's accumulator register i as the B operand of
//     the step over rows {i, 4 + i, 8 + i, 12 + i} of the tile: no cross-lane move, no LDS round trip. The
//     other operand is read from the image one fp32 per lane at (row 4g + i, column 16 dt + lr).
// LDS images are [256 rows][64 fp32] (256-byte rows) with the 16-byte chunks XOR-swizzled by row & 15: the 16
// lanes of a row-fragment read (16 rows, one chunk each) and the 64 lanes of a column read (4 rows x 16
// consecutive floats) each cover 16 / 64 distinct banks.
// Dropout: keep(b, h, q, key) = b2p_keep(seed, ((b*nh + h)*T + q)*TP + key), TP = T rounded up to even: the
// mask b2p_softmax_fwd draws, so the fused and unfused paths agree element for element. The backward
// rehashes (at the fp32 MFMA rate the hash hides behind the products).
// Every output element is written exactly once per launch, without atomics: runs repeat bit for bit.
#include "common.h"
#include <stdlib.h>
#include "../../include/b2p_hip.h"

namespace {
constexpr int DH = 64;       // head size
constexpr int TMAX = 256;    // keys / queries of one (batch, head)
constexpr int BLK = 128;     // queries (fwd, dQ) or keys (dK/dV) per workgroup
constexpr int TILE_B = 16 * DH * 4;   // bytes of a 16-row tile of an image
constexpr int IMG_B = TMAX * DH * 4;  // bytes of an image
constexpr float LOG2E = 1.4426950408889634f;

__device__ __forceinline__ f32x4 mfma(float a, float b, const f32x4& c) {
  return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}
__device__ __forceinline__ float exp2_fast(float x) { return __builtin_amdgcn_exp2f(x); }

// byte offset inside a 16-row tile of chunk 4g + j (floats 16g + 4j ..+3) of row lr
__device__ __forceinline__ int row_off(int lr, int g, int j) { return lr * 256 + (((4 * g + j) ^ lr) << 4); }
// byte offset inside a 16-row tile of the float at (row 4g + i, column 16 dt + lr)
__device__ __forceinline__ int col_off(int lr, int g, int i, int dt) {
  const int r = 4 * g + i;
  return r * 256 + (((4 * dt + (lr >> 2)) ^ r) << 4) + ((lr & 3) << 2);
}
// a lane's 16 operands of a product over the head dimension: floats 16g .. 16g + 15 of row lr of a tile
__device__ __forceinline__ void row_frag(const char* tile, const int (&ro)[4], float (&f)[16]) {
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const float4 v = *reinterpret_cast<const float4*>(tile + ro[j]);
    f[4 * j] = v.x; f[4 * j + 1] = v.y; f[4 * j + 2] = v.z; f[4 * j + 3] = v.w;
  }
}
// the same 16 operands of row `row` of a row-major global matrix (zeros when !ok)
__device__ __forceinline__ void grow_frag(const float* p, bool ok, float (&f)[16]) {
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (ok) v = *reinterpret_cast<const float4*>(p + 4 * j);
    f[4 * j] = v.x; f[4 * j + 1] = v.y; f[4 * j + 2] = v.z; f[4 * j + 3] = v.w;
  }
}
// Load rows [0, 256) of a head slice (64 fp32 at column `col` of a row-major [B*T][ld] matrix) into an LDS
// image; rows >= T are zero. 256 threads, 16 chunks of 16 B each.
__device__ __forceinline__ void load_image(char* img, const float* base, int64_t row0, int T, int64_t ld, int col,
                                           int tid) {
#pragma unroll
  for (int k = 0; k < TMAX / 16; ++k) {
    const int idx = tid + 256 * k;
    const int r = idx >> 4, c = idx & 15;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (r < T) v = *reinterpret_cast<const float4*>(base + (row0 + r) * ld + col + 4 * c);
    *reinterpret_cast<float4*>(img + r * 256 + ((c ^ (r & 15)) << 4)) = v;
  }
}
// zero rows [r0, r0 + 128) below T of a 64-column slice at column col of a row-major [B*T][ld] matrix
__device__ __forceinline__ void zero_block(float* dst, int64_t row0, int r0, int T, int64_t ld, int64_t col, int tid) {
  for (int i = tid; i < BLK * 16; i += 256) {
    const int r = r0 + (i >> 4);
    if (r < T) *reinterpret_cast<float4*>(dst + (row0 + r) * ld + col + 4 * (i & 15)) = make_float4(0.f, 0.f, 0.f, 0.f);
  }
}
__device__ __forceinline__ void zero_rows(float* dst, int64_t bh, int r0, int T, int tid) {
  for (int i = tid; i < BLK; i += 256)
    if (r0 + i < T) dst[bh * T + r0 + i] = 0.f;
}

struct DropCfg {
  uint64_t seed;
  uint32_t thr;
  float scale;                // 1 / (1 - p)
  const uint64_t* epoch;      // graph-replay seed offset (b2p_seed_eff), NULL in eager launches
  const int32_t* gate;        // LayerDrop gate (b2p_gate): closed -> zeros everywhere, no work
};

// the 4 keep bits of keys key0 .. key0+3 (key0 % 4 == 0; key_lo = 32-bit element index of key0, even row
// stride): b2p_keep's two 16-bit halves of two hashes (b2p_hash with idx >> 32 == 0, checked on the host)
__device__ __forceinline__ uint32_t keep4_bits(uint32_t key_lo, uint32_t k32, uint32_t thr16) {
#ifdef B2P_HASH_1R
  const uint32_t h0 = b2p_mix32((key_lo >> 1) ^ k32);
  const uint32_t h1 = b2p_mix32(((key_lo >> 1) + 1) ^ k32);
#else
  const uint32_t h0 = b2p_mix32(b2p_mix32((key_lo >> 1) ^ k32) + k32);
  const uint32_t h1 = b2p_mix32(b2p_mix32(((key_lo >> 1) + 1) ^ k32) + k32);
#endif
  return (uint32_t)((h0 & 0xFFFFu) >= thr16) | ((uint32_t)((h0 >> 16) >= thr16) << 1) |
         ((uint32_t)((h1 & 0xFFFFu) >= thr16) << 2) | ((uint32_t)((h1 >> 16) >= thr16) << 3);
}

// ------------------------------------------------------------------------------------------ forward
// qkv [B*T][3*D] fp32 (q | k | v, head-major inside each); O [B*T][D]; lse2 [B][nh][T]. One workgroup per
// (batch, head, 128-query block): 4 waves stage K and V once, then each wave runs query tiles w and w + 4.
template <bool DROP>
__global__ void __launch_bounds__(256) attn32_fwd_k(const float* __restrict__ qkv, float* __restrict__ O,
                                                    float* __restrict__ lse2, int T, int nh, float scale, DropCfg dc) {
  constexpr int NKT = TMAX / 16;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int nqb = (T + BLK - 1) / BLK;
  const int bh = blockIdx.x / nqb, qb = blockIdx.x - bh * nqb;
  const int b = bh / nh, h = bh - b * nh;
  const int D = nh * DH;
  const int64_t ld = 3 * (int64_t)D;
  const int tid = threadIdx.x, w = tid >> 6, l = tid & 63, lr = l & 15, g = l >> 4;
  const int64_t row0 = (int64_t)b * T;
  if (b2p_gated_off(dc.gate)) {   // LayerDrop: this replay skips the layer: O = 0, lse2 = 0 (finite)
    zero_block(O, row0, qb * BLK, T, D, h * DH, tid);
    zero_rows(lse2, bh, qb * BLK, T, tid);
    return;
  }
  dc.seed = b2p_seed_eff(dc.seed, dc.epoch);
  load_image(smem, qkv, row0, T, ld, D + h * DH, tid);
  load_image(smem + IMG_B, qkv, row0, T, ld, 2 * D + h * DH, tid);
  __syncthreads();
  const char* Kimg = smem;
  const char* Vimg = smem + IMG_B;
  int ro[4], co[4][4];
#pragma unroll
  for (int j = 0; j < 4; ++j) ro[j] = row_off(lr, g, j);
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) co[i][dt] = col_off(lr, g, i, dt);
  const float c2 = scale * LOG2E;
  const uint32_t k32 = (uint32_t)dc.seed ^ b2p_mix32((uint32_t)(dc.seed >> 32) + 0x9E3779B9u);   // b2p_hash key
  const uint32_t thr16 = b2p_thr16(dc.thr);
  const int TP = T + (T & 1);
  const int qt0 = qb * (BLK / 16) + w;
  for (int qt = qt0; qt < (qb + 1) * (BLK / 16) && qt * 16 < T; qt += 4) {
    const int q = qt * 16 + lr;
    const bool qok = q < T;
    float qf[16];
    grow_frag(qkv + (row0 + (qok ? q : 0)) * ld + h * DH + 16 * g, qok, qf);
    // S^T: tile kt = keys kt*16 + 4g + i (registers) x query q (lane); two tiles per pass (independent chains)
    f32x4 s[NKT];
#pragma unroll
    for (int kt = 0; kt < NKT; kt += 2) {
      float k0[16], k1[16];
      row_frag(Kimg + kt * TILE_B, ro, k0);
      row_frag(Kimg + (kt + 1) * TILE_B, ro, k1);
      s[kt] = s[kt + 1] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int st = 0; st < 16; ++st) {
        s[kt] = mfma(k0[st], qf[st], s[kt]);
        s[kt + 1] = mfma(k1[st], qf[st], s[kt + 1]);
      }
    }
    // row max of the raw scores (scale > 0 commutes with max); keys >= T -> -inf
    float m = -INFINITY;
#pragma unroll
    for (int kt = 0; kt < NKT; ++kt)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const float v = kt * 16 + 4 * g + i < T ? s[kt][i] : -INFINITY;
        s[kt][i] = v;
        m = fmaxf(m, v);
      }
    m = fmaxf(m, __shfl_xor(m, 16, 64));
    m = fmaxf(m, __shfl_xor(m, 32, 64));
    const float mc = m * c2;
    float sum = 0.f;
#pragma unroll
    for (int kt = 0; kt < NKT; ++kt)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const float e = exp2_fast(fmaf(s[kt][i], c2, -mc));
        s[kt][i] = e;
        sum += e;
      }
    sum += __shfl_xor(sum, 16, 64);
    sum += __shfl_xor(sum, 32, 64);
    const float inv = 1.f / sum;
    const uint32_t rowlo = ((uint32_t)bh * (uint32_t)T + (uint32_t)(qok ? q : 0)) * (uint32_t)TP;
    // O^T (d x q) = V^T (d x keys) . P_d^T (keys x q): step (kt, i) sums keys kt*16 + 4g' + i, g' = 0..3
    f32x4 o[4];
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) o[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int kt = 0; kt < NKT; ++kt) {
      const uint32_t kb = DROP ? keep4_bits(rowlo + (uint32_t)(kt * 16 + 4 * g), k32, thr16) : 0xFu;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        float pv = s[kt][i] * inv;
        if constexpr (DROP) pv = ((kb >> i) & 1u) ? pv * dc.scale : 0.f;
#pragma unroll
        for (int dt = 0; dt < 4; ++dt)
          o[dt] = mfma(*reinterpret_cast<const float*>(Vimg + kt * TILE_B + co[i][dt]), pv, o[dt]);
      }
    }
    if (qok) {
      float* orow = O + (row0 + q) * D + h * DH + 4 * g;
#pragma unroll
      for (int dt = 0; dt < 4; ++dt)
        *reinterpret_cast<float4*>(orow + dt * 16) = make_float4(o[dt][0], o[dt][1], o[dt][2], o[dt][3]);
      if (g == 0) lse2[(int64_t)bh * T + q] = mc + __log2f(sum);
    }
  }
}

// --------------------------------------------------------------------------------------- backward dQ
// Runs BEFORE the dK/dV kernel: delta[q] = sum_key P_d dP_d is formed here from the very P and dP the kernel
// recomputes, so sum_key dS = 0 holds to fp32 rounding. Pass 1 keeps P and dP*keep in registers, pass 2
// forms dS and dQ^T += K^T dS^T. One workgroup per (batch, head, 128 queries): K and V staged once.
template <bool DROP>
__global__ void __launch_bounds__(256) attn32_bwd_dq_k(const float* __restrict__ qkv, const float* __restrict__ dO,
                                                       const float* __restrict__ lse2, float* __restrict__ delta,
                                                       float* __restrict__ dqkv, int T, int nh, float scale,
                                                       DropCfg dc) {
  constexpr int NKT = TMAX / 16;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int nqb = (T + BLK - 1) / BLK;
  const int bh = blockIdx.x / nqb, qb = blockIdx.x - bh * nqb;
  const int b = bh / nh, h = bh - b * nh;
  const int D = nh * DH;
  const int64_t ld = 3 * (int64_t)D;
  const int tid = threadIdx.x, w = tid >> 6, l = tid & 63, lr = l & 15, g = l >> 4;
  const int64_t row0 = (int64_t)b * T;
  const int64_t nrows = (int64_t)(gridDim.x / nqb) * T;   // B * nh * T: the planes of delta_ws
  if (b2p_gated_off(dc.gate)) {   // LayerDrop: zero dQ and delta
    zero_block(dqkv, row0, qb * BLK, T, ld, h * DH, tid);
    zero_rows(delta, bh, qb * BLK, T, tid);
    zero_rows(delta + nrows, bh, qb * BLK, T, tid);
    return;
  }
  dc.seed = b2p_seed_eff(dc.seed, dc.epoch);
  load_image(smem, qkv, row0, T, ld, D + h * DH, tid);
  load_image(smem + IMG_B, qkv, row0, T, ld, 2 * D + h * DH, tid);
  __syncthreads();
  const char* Kimg = smem;
  const char* Vimg = smem + IMG_B;
  int ro[4], co[4][4];
#pragma unroll
  for (int j = 0; j < 4; ++j) ro[j] = row_off(lr, g, j);
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) co[i][dt] = col_off(lr, g, i, dt);
  const float c2 = scale * LOG2E;
  const uint32_t k32 = (uint32_t)dc.seed ^ b2p_mix32((uint32_t)(dc.seed >> 32) + 0x9E3779B9u);
  const uint32_t thr16 = b2p_thr16(dc.thr);
  const int TP = T + (T & 1);
  const int qt0 = qb * (BLK / 16) + w;
  for (int qt = qt0; qt < (qb + 1) * (BLK / 16) && qt * 16 < T; qt += 4) {
    const int q = qt * 16 + lr;
    const bool qok = q < T;
    float qf[16], df[16];
    grow_frag(qkv + (row0 + (qok ? q : 0)) * ld + h * DH + 16 * g, qok, qf);
    grow_frag(dO + (row0 + (qok ? q : 0)) * D + h * DH + 16 * g, qok, df);
    const int64_t rowc = (int64_t)bh * T + (qok ? q : 0);
    const float ls = qok ? lse2[rowc] : 0.f;
    const uint32_t rowlo = (uint32_t)rowc * (uint32_t)TP;
    // keys >= T are masked; rows q >= T need no mask (a lane's dS only reaches its own, unstored dQ row)
    f32x4 P[NKT], PD[NKT];
    float dl = 0.f, rs = 0.f;
#pragma unroll
    for (int kt = 0; kt < NKT; ++kt) {
      float kf[16], vf[16];
      row_frag(Kimg + kt * TILE_B, ro, kf);
      row_frag(Vimg + kt * TILE_B, ro, vf);
      f32x4 sv = f32x4{0.f, 0.f, 0.f, 0.f}, dp = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int st = 0; st < 16; ++st) {
        sv = mfma(kf[st], qf[st], sv);
        dp = mfma(vf[st], df[st], dp);
      }
      const uint32_t kb = DROP ? keep4_bits(rowlo + (uint32_t)(kt * 16 + 4 * g), k32, thr16) : 0xFu;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const bool ok = kt * 16 + 4 * g + i < T;
        const float p = ok ? exp2_fast(fmaf(sv[i], c2, -ls)) : 0.f;
        float pd = dp[i];
        if constexpr (DROP) pd = ((kb >> i) & 1u) ? pd * dc.scale : 0.f;
        pd = ok ? pd : 0.f;
        P[kt][i] = p;
        PD[kt][i] = pd;
        dl += p * pd;
        rs += p;
      }
    }
    dl += __shfl_xor(dl, 16, 64);
    dl += __shfl_xor(dl, 32, 64);
    rs += __shfl_xor(rs, 16, 64);
    rs += __shfl_xor(rs, 32, 64);
    // The recomputed row p = exp2(s - lse2) sums to rs = 1 + e, |e| up to ~6e-7: lse2 is one fp32 near 8 (its
    // ulp there is 9.5e-7 in the log2 domain) and the v_log_f32 / v_exp_f32 results carry an ulp each. A
    // row-coherent error of that size in P is ~6x the rounding noise of the unfused path's stored P, and the
    // full fine-tune's Adam trajectory (updates ~lr * sign(g)) follows it: measured 3.6e-5 / 2.0e-4 at steps
    // 2 / 3 of conformer_large_ft_bs8 in fp32 mode against 5.4e-6 / 6.4e-5 unfused. So both backward kernels
    // normalise p by the row sum this kernel forms: 1 / rs goes to the second plane of delta_ws for dK/dV,
    // delta is the normalised rows' (sum_key dS = 0 holds to rounding), dQ's own row is scaled at the store.
    const float irs = 1.f / rs;
    dl *= irs;
    if (qok && g == 0) {
      delta[rowc] = dl;
      delta[nrows + rowc] = irs;
    }
    f32x4 dq[4];
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) dq[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int kt = 0; kt < NKT; ++kt)
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const float ds = P[kt][i] * (PD[kt][i] - dl);
#pragma unroll
        for (int dt = 0; dt < 4; ++dt)
          dq[dt] = mfma(*reinterpret_cast<const float*>(Kimg + kt * TILE_B + co[i][dt]), ds, dq[dt]);
      }
    if (qok) {
      float* r = dqkv + (row0 + q) * ld + h * DH + 4 * g;
      const float qs = scale * irs;
#pragma unroll
      for (int dt = 0; dt < 4; ++dt)
        *reinterpret_cast<float4*>(r + dt * 16) =
            make_float4(dq[dt][0] * qs, dq[dt][1] * qs, dq[dt][2] * qs, dq[dt][3] * qs);
    }
  }
}

// ------------------------------------------------------------------------------------ backward dK dV
// delta_ws [2][B][nh][T] from the dQ kernel (delta, 1 / row sum); writes dK, dV into dqkv columns [D + h*64, ...) and [2D + h*64, ...).
// One workgroup per (batch, head, 128 keys): Q and dO are staged once (4 waves x key tiles w and w + 4).
template <bool DROP>
__global__ void __launch_bounds__(256) attn32_bwd_dkv_k(const float* __restrict__ qkv, const float* __restrict__ dO,
                                                        const float* __restrict__ lse2, const float* __restrict__ delta,
                                                        float* __restrict__ dqkv, int T, int nh, float scale,
                                                        DropCfg dc) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* lse_s = reinterpret_cast<float*>(smem + 2 * IMG_B);
  float* del_s = lse_s + TMAX;
  float* irs_s = del_s + TMAX;
  const int nkb = (T + BLK - 1) / BLK;
  const int bh = blockIdx.x / nkb, kb = blockIdx.x - bh * nkb;
  const int b = bh / nh, h = bh - b * nh;
  const int D = nh * DH;
  const int64_t ld = 3 * (int64_t)D;
  const int tid = threadIdx.x, w = tid >> 6, l = tid & 63, lr = l & 15, g = l >> 4;
  const int64_t row0 = (int64_t)b * T;
  if (b2p_gated_off(dc.gate)) {   // LayerDrop: zero dK, dV
    zero_block(dqkv, row0, kb * BLK, T, ld, D + h * DH, tid);
    zero_block(dqkv, row0, kb * BLK, T, ld, 2 * D + h * DH, tid);
    return;
  }
  dc.seed = b2p_seed_eff(dc.seed, dc.epoch);
  const int64_t nrows = (int64_t)(gridDim.x / nkb) * T;   // B * nh * T: the planes of delta_ws
  load_image(smem, qkv, row0, T, ld, h * DH, tid);
  load_image(smem + IMG_B, dO, row0, T, D, h * DH, tid);
  for (int qq = tid; qq < TMAX; qq += 256) {
    const int64_t o = (int64_t)bh * T + qq;
    lse_s[qq] = qq < T ? lse2[o] : 0.f;
    del_s[qq] = qq < T ? delta[o] : 0.f;
    irs_s[qq] = qq < T ? delta[nrows + o] : 0.f;
  }
  __syncthreads();
  const char* Qimg = smem;
  const char* dOimg = smem + IMG_B;
  int ro[4], co[4][4];
#pragma unroll
  for (int j = 0; j < 4; ++j) ro[j] = row_off(lr, g, j);
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) co[i][dt] = col_off(lr, g, i, dt);
  const float c2 = scale * LOG2E;
  const int TP = T + (T & 1);
  const int nqt = (T + 15) >> 4;
  const int kt0 = kb * (BLK / 16) + w;
  for (int kt = kt0; kt < (kb + 1) * (BLK / 16) && kt * 16 < T; kt += 4) {
    const int key = kt * 16 + lr;
    const bool kok = key < T;
    float kf[16], vf[16];
    grow_frag(qkv + (row0 + (kok ? key : 0)) * ld + D + h * DH + 16 * g, kok, kf);
    grow_frag(qkv + (row0 + (kok ? key : 0)) * ld + 2 * D + h * DH + 16 * g, kok, vf);
    f32x4 dv[4], dk[4];
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) dv[dt] = dk[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int qt = 0; qt < nqt; ++qt) {
      const char* Qt = Qimg + qt * TILE_B;
      const char* dOt = dOimg + qt * TILE_B;
      float qf[16], of[16];
      row_frag(Qt, ro, qf);
      row_frag(dOt, ro, of);
      // rows q = qt*16 + 4g + i (registers), column key (lane)
      f32x4 sv = f32x4{0.f, 0.f, 0.f, 0.f}, dp = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int st = 0; st < 16; ++st) {
        sv = mfma(qf[st], kf[st], sv);
        dp = mfma(of[st], vf[st], dp);
      }
      const int qb = qt * 16 + 4 * g;
      const float4 ls4 = *reinterpret_cast<const float4*>(lse_s + qb);
      const float4 dl4 = *reinterpret_cast<const float4*>(del_s + qb);
      const float4 ir4 = *reinterpret_cast<const float4*>(irs_s + qb);
      const float lsv[4] = {ls4.x, ls4.y, ls4.z, ls4.w}, dlv[4] = {dl4.x, dl4.y, dl4.z, dl4.w};
      const float irv[4] = {ir4.x, ir4.y, ir4.z, ir4.w};
      float pd[4], ds[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        // queries >= T are masked; a key >= T needs no mask (its column only reaches its own, unstored rows)
        const float p = qb + i < T ? exp2_fast(fmaf(sv[i], c2, -lsv[i])) * irv[i] : 0.f;   // over the row sum (dQ pass)
        float ksc = 1.f;
        if constexpr (DROP)
          ksc = b2p_keep(dc.seed, ((uint64_t)bh * T + (uint64_t)(qb + i)) * (uint64_t)TP + (uint64_t)key, dc.thr)
                    ? dc.scale : 0.f;
        pd[i] = p * ksc;
        ds[i] = p * (dp[i] * ksc - dlv[i]);
      }
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) {
          dv[dt] = mfma(*reinterpret_cast<const float*>(dOt + co[i][dt]), pd[i], dv[dt]);
          dk[dt] = mfma(*reinterpret_cast<const float*>(Qt + co[i][dt]), ds[i], dk[dt]);
        }
    }
    if (kok) {
      float* r = dqkv + (row0 + key) * ld + h * DH + 4 * g;
#pragma unroll
      for (int dt = 0; dt < 4; ++dt) {
        *reinterpret_cast<float4*>(r + D + dt * 16) =
            make_float4(dk[dt][0] * scale, dk[dt][1] * scale, dk[dt][2] * scale, dk[dt][3] * scale);
        *reinterpret_cast<float4*>(r + 2 * D + dt * 16) = make_float4(dv[dt][0], dv[dt][1], dv[dt][2], dv[dt][3]);
      }
    }
  }
}

// ================================================================== long class: 257 <= T' <= 512
// A 512-row fp32 image is 128 KB, so K and V (backward: Q and dO) of a head are staged as two 256-row chunks,
// one after the other, into the same two 64 KB images; fragments, swizzle and work split are the 256 class's.
// Only the 32-row tile pairs that hold a row < T are staged and visited (T' = 313: 2 of the second chunk's 8).
constexpr int TLONG = 512;
constexpr int NCH = TLONG / TMAX;   // chunks

// Rows [r0, r0 + 256) of a head slice into an LDS image (load_image's layout): only the 32-row tile pairs
// with a row < T are written, rows >= T inside them are zero.
__device__ __forceinline__ void load_chunk(char* img, const float* base, int64_t row0, int r0, int T, int64_t ld,
                                           int col, int tid) {
#pragma unroll
  for (int k = 0; k < TMAX / 16; ++k) {
    const int idx = tid + 256 * k;
    const int r = idx >> 4, c = idx & 15;
    if (r0 + (r & ~31) < T) {
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (r0 + r < T) v = *reinterpret_cast<const float4*>(base + (row0 + r0 + r) * ld + col + 4 * c);
      *reinterpret_cast<float4*>(img + r * 256 + ((c ^ (r & 15)) << 4)) = v;
    }
  }
}

// ------------------------------------------------------------------------------------------ forward
// One workgroup per (batch, head, 128-query block); each wave keeps its two query tiles' running max, running
// sum and unnormalised O^T accumulators across the chunks (online softmax: a chunk rescales them by
// exp2(m_old - m_new)) and divides by the sum at the store.
template <bool DROP>
__global__ void __launch_bounds__(256) attn32_long_fwd_k(const float* __restrict__ qkv, float* __restrict__ O,
                                                         float* __restrict__ lse2, int T, int nh, float scale,
                                                         DropCfg dc) {
  constexpr int NKT = TMAX / 16;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int nqb = (T + BLK - 1) / BLK;
  const int bh = blockIdx.x / nqb, qb = blockIdx.x - bh * nqb;
  const int b = bh / nh, h = bh - b * nh;
  const int D = nh * DH;
  const int64_t ld = 3 * (int64_t)D;
  const int tid = threadIdx.x, w = tid >> 6, l = tid & 63, lr = l & 15, g = l >> 4;
  const int64_t row0 = (int64_t)b * T;
  if (b2p_gated_off(dc.gate)) {   // LayerDrop: this replay skips the layer: O = 0, lse2 = 0 (finite)
    zero_block(O, row0, qb * BLK, T, D, h * DH, tid);
    zero_rows(lse2, bh, qb * BLK, T, tid);
    return;
  }
  dc.seed = b2p_seed_eff(dc.seed, dc.epoch);
  const char* Kimg = smem;
  const char* Vimg = smem + IMG_B;
  int ro[4], co[4][4];
#pragma unroll
  for (int j = 0; j < 4; ++j) ro[j] = row_off(lr, g, j);
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) co[i][dt] = col_off(lr, g, i, dt);
  const float c2 = scale * LOG2E;
  const uint32_t k32 = (uint32_t)dc.seed ^ b2p_mix32((uint32_t)(dc.seed >> 32) + 0x9E3779B9u);   // b2p_hash key
  const uint32_t thr16 = b2p_thr16(dc.thr);
  const int TP = T + (T & 1);
  float mrun[2], lrun[2];
  f32x4 o[2][4];
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    mrun[j] = -INFINITY;
    lrun[j] = 0.f;
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) o[j][dt] = f32x4{0.f, 0.f, 0.f, 0.f};
  }
  for (int c = 0; c < NCH; ++c) {
    const int r0 = c * TMAX;
    const int Tc = T - r0;   // keys of this chunk below T (every chunk holds one: T > 256)
    if (c) __syncthreads();  // every wave is done with the previous chunk's images
    load_chunk(smem, qkv, row0, r0, T, ld, D + h * DH, tid);
    load_chunk(smem + IMG_B, qkv, row0, r0, T, ld, 2 * D + h * DH, tid);
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int qt = qb * (BLK / 16) + w + 4 * j;
      if (qt * 16 >= T) continue;
      const int q = qt * 16 + lr;
      const bool qok = q < T;
      float qf[16];
      grow_frag(qkv + (row0 + (qok ? q : 0)) * ld + h * DH + 16 * g, qok, qf);
      // S^T of the chunk: tile kt = keys r0 + kt*16 + 4g + i (registers) x query q (lane)
      f32x4 s[NKT];
#pragma unroll
      for (int kt = 0; kt < NKT; kt += 2) {
        s[kt] = s[kt + 1] = f32x4{0.f, 0.f, 0.f, 0.f};
        if (kt * 16 < Tc) {
          float k0[16], k1[16];
          row_frag(Kimg + kt * TILE_B, ro, k0);
          row_frag(Kimg + (kt + 1) * TILE_B, ro, k1);
#pragma unroll
          for (int st = 0; st < 16; ++st) {
            s[kt] = mfma(k0[st], qf[st], s[kt]);
            s[kt + 1] = mfma(k1[st], qf[st], s[kt + 1]);
          }
        }
      }
      float m = -INFINITY;
#pragma unroll
      for (int kt = 0; kt < NKT; ++kt)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const float v = kt * 16 + 4 * g + i < Tc ? s[kt][i] : -INFINITY;
          s[kt][i] = v;
          m = fmaxf(m, v);
        }
      m = fmaxf(m, __shfl_xor(m, 16, 64));
      m = fmaxf(m, __shfl_xor(m, 32, 64));
      m = fmaxf(m, mrun[j]);
      const float mc = m * c2;
      const float alpha = exp2_fast((mrun[j] - m) * c2);   // first chunk: exp2(-inf) = 0 over zeros
      mrun[j] = m;
      float sum = 0.f;
#pragma unroll
      for (int kt = 0; kt < NKT; ++kt)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const float e = exp2_fast(fmaf(s[kt][i], c2, -mc));   // keys >= T: exp2(-inf) = 0
          s[kt][i] = e;
          sum += e;
        }
      sum += __shfl_xor(sum, 16, 64);
      sum += __shfl_xor(sum, 32, 64);
      lrun[j] = fmaf(lrun[j], alpha, sum);
#pragma unroll
      for (int dt = 0; dt < 4; ++dt)
#pragma unroll
        for (int i = 0; i < 4; ++i) o[j][dt][i] *= alpha;
      const uint32_t rowlo = ((uint32_t)bh * (uint32_t)T + (uint32_t)(qok ? q : 0)) * (uint32_t)TP + (uint32_t)r0;
      // O^T (d x q) += V_c^T (d x keys) . E_d^T (keys x q), E = exp2(s - m) unnormalised
#pragma unroll
      for (int kt = 0; kt < NKT; ++kt) {
        if (kt * 16 >= Tc) continue;
        const uint32_t kb = DROP ? keep4_bits(rowlo + (uint32_t)(kt * 16 + 4 * g), k32, thr16) : 0xFu;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          float pv = s[kt][i];
          if constexpr (DROP) pv = ((kb >> i) & 1u) ? pv * dc.scale : 0.f;
#pragma unroll
          for (int dt = 0; dt < 4; ++dt)
            o[j][dt] = mfma(*reinterpret_cast<const float*>(Vimg + kt * TILE_B + co[i][dt]), pv, o[j][dt]);
        }
      }
    }
  }
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int q = (qb * (BLK / 16) + w + 4 * j) * 16 + lr;
    if (q < T) {
      const float inv = 1.f / lrun[j];
      float* orow = O + (row0 + q) * D + h * DH + 4 * g;
#pragma unroll
      for (int dt = 0; dt < 4; ++dt)
        *reinterpret_cast<float4*>(orow + dt * 16) =
            make_float4(o[j][dt][0] * inv, o[j][dt][1] * inv, o[j][dt][2] * inv, o[j][dt][3] * inv);
      if (g == 0) lse2[(int64_t)bh * T + q] = fmaf(mrun[j], c2, __log2f(lrun[j]));
    }
  }
}

// --------------------------------------------------------------------------------------- backward dQ
// One query tile's visit of the staged chunk: S^T and dP^T tiles, P = exp2(s - lse2), dP_d = dP * keep.
// SECOND = false: accumulates the lane's parts of sum_key P dP_d and of the row sum. SECOND = true: dS =
// P (dP_d - dl) with the finished dl, dQ^T += K_c^T dS^T.
template <bool DROP, bool SECOND>
__device__ __forceinline__ void long_dq_tile(const char* Kimg, const char* Vimg, const int (&ro)[4],
                                             const int (&co)[4][4], const float (&qf)[16], const float (&df)[16],
                                             float ls, uint32_t rowlo, int Tc, int g, float c2, uint32_t k32,
                                             uint32_t thr16, float dscale, float& dl, float& rs, f32x4 (&dq)[4]) {
  const int nkt = Tc < TMAX ? (Tc + 15) >> 4 : TMAX / 16;
  for (int kt = 0; kt < nkt; ++kt) {
    float kf[16], vf[16];
    row_frag(Kimg + kt * TILE_B, ro, kf);
    row_frag(Vimg + kt * TILE_B, ro, vf);
    f32x4 sv = f32x4{0.f, 0.f, 0.f, 0.f}, dp = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int st = 0; st < 16; ++st) {
      sv = mfma(kf[st], qf[st], sv);
      dp = mfma(vf[st], df[st], dp);
    }
    const uint32_t kb = DROP ? keep4_bits(rowlo + (uint32_t)(kt * 16 + 4 * g), k32, thr16) : 0xFu;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const bool ok = kt * 16 + 4 * g + i < Tc;
      const float p = ok ? exp2_fast(fmaf(sv[i], c2, -ls)) : 0.f;
      float pd = dp[i];
      if constexpr (DROP) pd = ((kb >> i) & 1u) ? pd * dscale : 0.f;
      pd = ok ? pd : 0.f;
      if constexpr (!SECOND) {
        dl += p * pd;
        rs += p;
      } else {
        const float ds = p * (pd - dl);
#pragma unroll
        for (int dt = 0; dt < 4; ++dt)
          dq[dt] = mfma(*reinterpret_cast<const float*>(Kimg + kt * TILE_B + co[i][dt]), ds, dq[dt]);
      }
    }
  }
}

// Runs BEFORE the dK/dV kernel, as in the 256 class, and keeps its property: delta and the row sum come from
// the very P and dP this kernel recomputes, and P is divided by that row sum (the comment in attn32_bwd_dq_k).
// delta over all keys is needed before any dS and a row's 512 P and dP do not fit in registers beside a
// second tile's, so the chunks are swept twice: (chunk 0, chunk 1) for the row constants, then (chunk 1, still
// staged, chunk 0) for dQ: three stagings, and S^T / dP^T computed twice.
template <bool DROP>
__global__ void __launch_bounds__(256) attn32_long_bwd_dq_k(const float* __restrict__ qkv,
                                                            const float* __restrict__ dO,
                                                            const float* __restrict__ lse2, float* __restrict__ delta,
                                                            float* __restrict__ dqkv, int T, int nh, float scale,
                                                            DropCfg dc) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int nqb = (T + BLK - 1) / BLK;
  const int bh = blockIdx.x / nqb, qb = blockIdx.x - bh * nqb;
  const int b = bh / nh, h = bh - b * nh;
  const int D = nh * DH;
  const int64_t ld = 3 * (int64_t)D;
  const int tid = threadIdx.x, w = tid >> 6, l = tid & 63, lr = l & 15, g = l >> 4;
  const int64_t row0 = (int64_t)b * T;
  const int64_t nrows = (int64_t)(gridDim.x / nqb) * T;   // B * nh * T: the planes of delta_ws
  if (b2p_gated_off(dc.gate)) {   // LayerDrop: zero dQ and delta
    zero_block(dqkv, row0, qb * BLK, T, ld, h * DH, tid);
    zero_rows(delta, bh, qb * BLK, T, tid);
    zero_rows(delta + nrows, bh, qb * BLK, T, tid);
    return;
  }
  dc.seed = b2p_seed_eff(dc.seed, dc.epoch);
  const char* Kimg = smem;
  const char* Vimg = smem + IMG_B;
  int ro[4], co[4][4];
#pragma unroll
  for (int j = 0; j < 4; ++j) ro[j] = row_off(lr, g, j);
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) co[i][dt] = col_off(lr, g, i, dt);
  const float c2 = scale * LOG2E;
  const uint32_t k32 = (uint32_t)dc.seed ^ b2p_mix32((uint32_t)(dc.seed >> 32) + 0x9E3779B9u);
  const uint32_t thr16 = b2p_thr16(dc.thr);
  const int TP = T + (T & 1);
  float dl[2] = {0.f, 0.f}, rs[2] = {0.f, 0.f}, irs[2] = {0.f, 0.f};
  f32x4 dq[2][4];
#pragma unroll
  for (int j = 0; j < 2; ++j)
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) dq[j][dt] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int ph = 0; ph < 2 * NCH; ++ph) {   // (sweep, chunk): (0, 0) (0, 1) (1, 1) (1, 0)
    const int c = (ph == 1 || ph == 2) ? 1 : 0;
    const int r0 = c * TMAX;
    if (ph != 2) {
      if (ph) __syncthreads();   // every wave is done with the staged chunk
      load_chunk(smem, qkv, row0, r0, T, ld, D + h * DH, tid);
      load_chunk(smem + IMG_B, qkv, row0, r0, T, ld, 2 * D + h * DH, tid);
      __syncthreads();
    }
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int qt = qb * (BLK / 16) + w + 4 * j;
      if (qt * 16 >= T) continue;
      const int q = qt * 16 + lr;
      const bool qok = q < T;
      float qf[16], df[16];
      grow_frag(qkv + (row0 + (qok ? q : 0)) * ld + h * DH + 16 * g, qok, qf);
      grow_frag(dO + (row0 + (qok ? q : 0)) * D + h * DH + 16 * g, qok, df);
      const int64_t rowc = (int64_t)bh * T + (qok ? q : 0);
      const float ls = qok ? lse2[rowc] : 0.f;
      const uint32_t rowlo = (uint32_t)rowc * (uint32_t)TP + (uint32_t)r0;
      // keys >= T are masked; rows q >= T need no mask (a lane's dS only reaches its own, unstored dQ row)
      if (ph < 2) {
        long_dq_tile<DROP, false>(Kimg, Vimg, ro, co, qf, df, ls, rowlo, T - r0, g, c2, k32, thr16, dc.scale, dl[j],
                                  rs[j], dq[j]);
        if (ph == 1) {   // both chunks seen: the row constants (attn32_bwd_dq_k's, over all keys)
          float d = dl[j], r = rs[j];
          d += __shfl_xor(d, 16, 64);
          d += __shfl_xor(d, 32, 64);
          r += __shfl_xor(r, 16, 64);
          r += __shfl_xor(r, 32, 64);
          irs[j] = 1.f / r;
          dl[j] = d * irs[j];
          if (qok && g == 0) {
            delta[rowc] = dl[j];
            delta[nrows + rowc] = irs[j];
          }
        }
      } else {
        long_dq_tile<DROP, true>(Kimg, Vimg, ro, co, qf, df, ls, rowlo, T - r0, g, c2, k32, thr16, dc.scale, dl[j],
                                 rs[j], dq[j]);
      }
    }
  }
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int q = (qb * (BLK / 16) + w + 4 * j) * 16 + lr;
    if (q < T) {
      float* r = dqkv + (row0 + q) * ld + h * DH + 4 * g;
      const float qs = scale * irs[j];
#pragma unroll
      for (int dt = 0; dt < 4; ++dt)
        *reinterpret_cast<float4*>(r + dt * 16) =
            make_float4(dq[j][dt][0] * qs, dq[j][dt][1] * qs, dq[j][dt][2] * qs, dq[j][dt][3] * qs);
    }
  }
}

// ------------------------------------------------------------------------------------ backward dK dV
// One workgroup per (batch, head, 128 keys), the key on the lane: each wave keeps its two key tiles' dK^T and
// dV^T accumulators across the two staged chunks of Q and dO. The row constants of all T queries (lse2 and the
// dQ kernel's two planes) sit in LDS beside the images.
template <bool DROP>
__global__ void __launch_bounds__(256) attn32_long_bwd_dkv_k(const float* __restrict__ qkv,
                                                             const float* __restrict__ dO,
                                                             const float* __restrict__ lse2,
                                                             const float* __restrict__ delta,
                                                             float* __restrict__ dqkv, int T, int nh, float scale,
                                                             DropCfg dc) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* lse_s = reinterpret_cast<float*>(smem + 2 * IMG_B);
  float* del_s = lse_s + TLONG;
  float* irs_s = del_s + TLONG;
  const int nkb = (T + BLK - 1) / BLK;
  const int bh = blockIdx.x / nkb, kb = blockIdx.x - bh * nkb;
  const int b = bh / nh, h = bh - b * nh;
  const int D = nh * DH;
  const int64_t ld = 3 * (int64_t)D;
  const int tid = threadIdx.x, w = tid >> 6, l = tid & 63, lr = l & 15, g = l >> 4;
  const int64_t row0 = (int64_t)b * T;
  if (b2p_gated_off(dc.gate)) {   // LayerDrop: zero dK, dV
    zero_block(dqkv, row0, kb * BLK, T, ld, D + h * DH, tid);
    zero_block(dqkv, row0, kb * BLK, T, ld, 2 * D + h * DH, tid);
    return;
  }
  dc.seed = b2p_seed_eff(dc.seed, dc.epoch);
  const int64_t nrows = (int64_t)(gridDim.x / nkb) * T;   // B * nh * T: the planes of delta_ws
  for (int qq = tid; qq < TLONG; qq += 256) {
    const int64_t o = (int64_t)bh * T + qq;
    lse_s[qq] = qq < T ? lse2[o] : 0.f;
    del_s[qq] = qq < T ? delta[o] : 0.f;
    irs_s[qq] = qq < T ? delta[nrows + o] : 0.f;
  }
  const char* Qimg = smem;
  const char* dOimg = smem + IMG_B;
  int ro[4], co[4][4];
#pragma unroll
  for (int j = 0; j < 4; ++j) ro[j] = row_off(lr, g, j);
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) co[i][dt] = col_off(lr, g, i, dt);
  const float c2 = scale * LOG2E;
  const int TP = T + (T & 1);
  f32x4 dv[2][4], dk[2][4];
#pragma unroll
  for (int j = 0; j < 2; ++j)
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) dv[j][dt] = dk[j][dt] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int c = 0; c < NCH; ++c) {
    const int r0 = c * TMAX;
    if (c) __syncthreads();   // every wave is done with the previous chunk's images
    load_chunk(smem, qkv, row0, r0, T, ld, h * DH, tid);
    load_chunk(smem + IMG_B, dO, row0, r0, T, D, h * DH, tid);
    __syncthreads();
    const int nqt = T - r0 < TMAX ? (T - r0 + 15) >> 4 : TMAX / 16;
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int kt = kb * (BLK / 16) + w + 4 * j;
      if (kt * 16 >= T) continue;
      const int key = kt * 16 + lr;
      const bool kok = key < T;
      float kf[16], vf[16];
      grow_frag(qkv + (row0 + (kok ? key : 0)) * ld + D + h * DH + 16 * g, kok, kf);
      grow_frag(qkv + (row0 + (kok ? key : 0)) * ld + 2 * D + h * DH + 16 * g, kok, vf);
      for (int qt = 0; qt < nqt; ++qt) {
        const char* Qt = Qimg + qt * TILE_B;
        const char* dOt = dOimg + qt * TILE_B;
        float qf[16], of[16];
        row_frag(Qt, ro, qf);
        row_frag(dOt, ro, of);
        // rows q = r0 + qt*16 + 4g + i (registers), column key (lane)
        f32x4 sv = f32x4{0.f, 0.f, 0.f, 0.f}, dp = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int st = 0; st < 16; ++st) {
          sv = mfma(qf[st], kf[st], sv);
          dp = mfma(of[st], vf[st], dp);
        }
        const int q0 = r0 + qt * 16 + 4 * g;
        const float4 ls4 = *reinterpret_cast<const float4*>(lse_s + q0);
        const float4 dl4 = *reinterpret_cast<const float4*>(del_s + q0);
        const float4 ir4 = *reinterpret_cast<const float4*>(irs_s + q0);
        const float lsv[4] = {ls4.x, ls4.y, ls4.z, ls4.w}, dlv[4] = {dl4.x, dl4.y, dl4.z, dl4.w};
        const float irv[4] = {ir4.x, ir4.y, ir4.z, ir4.w};
        float pd[4], ds[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          // queries >= T are masked; a key >= T needs no mask (its column only reaches its own, unstored rows)
          const float p = q0 + i < T ? exp2_fast(fmaf(sv[i], c2, -lsv[i])) * irv[i] : 0.f;   // over the row sum (dQ pass)
          float ksc = 1.f;
          if constexpr (DROP)
            ksc = b2p_keep(dc.seed, ((uint64_t)bh * T + (uint64_t)(q0 + i)) * (uint64_t)TP + (uint64_t)key, dc.thr)
                      ? dc.scale : 0.f;
          pd[i] = p * ksc;
          ds[i] = p * (dp[i] * ksc - dlv[i]);
        }
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int dt = 0; dt < 4; ++dt) {
            dv[j][dt] = mfma(*reinterpret_cast<const float*>(dOt + co[i][dt]), pd[i], dv[j][dt]);
            dk[j][dt] = mfma(*reinterpret_cast<const float*>(Qt + co[i][dt]), ds[i], dk[j][dt]);
          }
      }
    }
  }
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int key = (kb * (BLK / 16) + w + 4 * j) * 16 + lr;
    if (key < T) {
      float* r = dqkv + (row0 + key) * ld + h * DH + 4 * g;
#pragma unroll
      for (int dt = 0; dt < 4; ++dt) {
        *reinterpret_cast<float4*>(r + D + dt * 16) =
            make_float4(dk[j][dt][0] * scale, dk[j][dt][1] * scale, dk[j][dt][2] * scale, dk[j][dt][3] * scale);
        *reinterpret_cast<float4*>(r + 2 * D + dt * 16) =
            make_float4(dv[j][dt][0], dv[j][dt][1], dv[j][dt][2], dv[j][dt][3]);
      }
    }
  }
}

DropCfg drop_cfg(float p, uint64_t seed) {
  DropCfg d;
  d.epoch = b2p_seed_epoch();
  d.gate = b2p_gate();
  d.seed = seed;
  d.thr = b2p_dropout_threshold(p);
  d.scale = p > 0.f ? 1.f / (1.f - p) : 1.f;
  return d;
}
constexpr size_t FWD_LDS = 2 * IMG_B;
constexpr size_t DKV_LDS = 2 * IMG_B + 3 * TMAX * 4;
constexpr size_t LONG_DKV_LDS = 2 * IMG_B + 3 * TLONG * 4;

template <typename K>
int set_lds(K kern, size_t bytes) {
  B2P_CHECK_HIP(hipFuncSetAttribute((const void*)kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
  return 0;
}
int init_attrs() {
  static int done = -1;
  if (done >= 0) return done;
  int rc = 0;
  rc |= set_lds(attn32_fwd_k<false>, FWD_LDS);
  rc |= set_lds(attn32_fwd_k<true>, FWD_LDS);
  rc |= set_lds(attn32_bwd_dq_k<false>, FWD_LDS);
  rc |= set_lds(attn32_bwd_dq_k<true>, FWD_LDS);
  rc |= set_lds(attn32_bwd_dkv_k<false>, DKV_LDS);
  rc |= set_lds(attn32_bwd_dkv_k<true>, DKV_LDS);
  rc |= set_lds(attn32_long_fwd_k<false>, FWD_LDS);
  rc |= set_lds(attn32_long_fwd_k<true>, FWD_LDS);
  rc |= set_lds(attn32_long_bwd_dq_k<false>, FWD_LDS);
  rc |= set_lds(attn32_long_bwd_dq_k<true>, FWD_LDS);
  rc |= set_lds(attn32_long_bwd_dkv_k<false>, LONG_DKV_LDS);
  rc |= set_lds(attn32_long_bwd_dkv_k<true>, LONG_DKV_LDS);
  done = rc;
  return done;
}
bool aligned16(const void* p) { return ((uintptr_t)p & 15u) == 0; }
}  // namespace

extern "C" int b2p_attn32_supported(int64_t T, int64_t dh) { return dh == DH && T >= 1 && T <= TMAX ? 1 : 0; }

extern "C" int b2p_attn32_fwd(const float* qkv, float* O, float* lse2, int64_t B, int64_t T, int64_t nh, int64_t dh,
                              float scale, float drop_p, uint64_t drop_seed, b2p_stream_t stream) {
  B2P_CHECK_ARG(qkv && O && lse2, "attn32_fwd: NULL pointer");
  B2P_CHECK_ARG(aligned16(qkv) && aligned16(O), "attn32_fwd: qkv and O must be 16-byte aligned");
  B2P_CHECK_ARG(b2p_attn32_supported(T, dh) && nh > 0, "attn32_fwd: needs head size 64, 1 <= T <= 256, heads > 0");
  B2P_CHECK_ARG(drop_p >= 0.f && drop_p < 1.f, "attn32_fwd: needs 0 <= drop_p < 1");
  if (B <= 0) return 0;
  B2P_CHECK_ARG(B * nh * T * (T + (T & 1)) < (1ll << 32), "attn32_fwd: B * heads * T * T must stay below 2^32 "
                "(32-bit dropout element index)");
  if (init_attrs()) return 2;
  const dim3 grid((unsigned)(B * nh * ((T + BLK - 1) / BLK)));
  const DropCfg dc = drop_cfg(drop_p, drop_seed);
  if (drop_p > 0.f)
    hipLaunchKernelGGL(attn32_fwd_k<true>, grid, dim3(256), FWD_LDS, (hipStream_t)stream, qkv, O, lse2, (int)T, (int)nh,
                       scale, dc);
  else
    hipLaunchKernelGGL(attn32_fwd_k<false>, grid, dim3(256), FWD_LDS, (hipStream_t)stream, qkv, O, lse2, (int)T, (int)nh,
                       scale, dc);
  B2P_CHECK_LAUNCH();
  return 0;
}

extern "C" int b2p_attn32_bwd(const float* qkv, const float* dO, const float* lse2, float* delta_ws, float* dqkv,
                              int64_t B, int64_t T, int64_t nh, int64_t dh, float scale, float drop_p,
                              uint64_t drop_seed, b2p_stream_t stream) {
  B2P_CHECK_ARG(qkv && dO && lse2 && delta_ws && dqkv, "attn32_bwd: NULL pointer");
  B2P_CHECK_ARG(aligned16(qkv) && aligned16(dO) && aligned16(dqkv), "attn32_bwd: qkv, dO and dqkv must be 16-byte aligned");
  B2P_CHECK_ARG(b2p_attn32_supported(T, dh) && nh > 0, "attn32_bwd: needs head size 64, 1 <= T <= 256, heads > 0");
  B2P_CHECK_ARG(drop_p >= 0.f && drop_p < 1.f, "attn32_bwd: needs 0 <= drop_p < 1");
  if (B <= 0) return 0;
  B2P_CHECK_ARG(B * nh * T * (T + (T & 1)) < (1ll << 32), "attn32_bwd: B * heads * T * T must stay below 2^32 "
                "(32-bit dropout element index)");
  if (init_attrs()) return 2;
  const dim3 grid((unsigned)(B * nh * ((T + BLK - 1) / BLK)));
  const DropCfg dc = drop_cfg(drop_p, drop_seed);
  hipStream_t st = (hipStream_t)stream;
  if (drop_p > 0.f) {
    hipLaunchKernelGGL(attn32_bwd_dq_k<true>, grid, dim3(256), FWD_LDS, st, qkv, dO, lse2, delta_ws, dqkv, (int)T, (int)nh,
                       scale, dc);
    hipLaunchKernelGGL(attn32_bwd_dkv_k<true>, grid, dim3(256), DKV_LDS, st, qkv, dO, lse2, delta_ws, dqkv, (int)T,
                       (int)nh, scale, dc);
  } else {
    hipLaunchKernelGGL(attn32_bwd_dq_k<false>, grid, dim3(256), FWD_LDS, st, qkv, dO, lse2, delta_ws, dqkv, (int)T,
                       (int)nh, scale, dc);
    hipLaunchKernelGGL(attn32_bwd_dkv_k<false>, grid, dim3(256), DKV_LDS, st, qkv, dO, lse2, delta_ws, dqkv, (int)T,
                       (int)nh, scale, dc);
  }
  B2P_CHECK_LAUNCH();
  return 0;
}

// ------------------------------------------------------------------ long class: 257 <= T <= 512 (b2p_hip.h)
extern "C" int b2p_attn32_long_supported(int64_t T, int64_t dh) { return dh == DH && T > TMAX && T <= TLONG ? 1 : 0; }

namespace {
// the shape and range checks both long-class calls share (1: rejected, the error is set)
int long_args(const char* what, int64_t B, int64_t T, int64_t nh, int64_t dh, float drop_p) {
  B2P_CHECK_ARG(dh == DH, "%s: needs head size 64", what);
  B2P_CHECK_ARG(T > TMAX && T <= TLONG, "%s: needs 257 <= T <= 512 (b2p_attn32_fwd / _bwd serve T <= 256)", what);
  B2P_CHECK_ARG(nh > 0, "%s: needs heads > 0", what);
  B2P_CHECK_ARG(drop_p >= 0.f && drop_p < 1.f, "%s: needs 0 <= drop_p < 1", what);
  B2P_CHECK_ARG(B <= 0 || B * nh * T * (T + (T & 1)) < (1ll << 32), "%s: B * heads * T * T must stay below 2^32 "
                "(32-bit dropout element index)", what);
  return 0;
}
}  // namespace

extern "C" int b2p_attn32_long_fwd(const float* qkv, float* O, float* lse2, int64_t B, int64_t T, int64_t nh,
                                   int64_t dh, float scale, float drop_p, uint64_t drop_seed, b2p_stream_t stream) {
  B2P_CHECK_ARG(qkv && O && lse2, "attn32_long_fwd: NULL pointer");
  B2P_CHECK_ARG(aligned16(qkv) && aligned16(O), "attn32_long_fwd: qkv and O must be 16-byte aligned");
  if (long_args("attn32_long_fwd", B, T, nh, dh, drop_p)) return 1;
  if (B <= 0) return 0;
  if (init_attrs()) return 2;
  const dim3 grid((unsigned)(B * nh * ((T + BLK - 1) / BLK)));
  const DropCfg dc = drop_cfg(drop_p, drop_seed);
  if (drop_p > 0.f)
    hipLaunchKernelGGL(attn32_long_fwd_k<true>, grid, dim3(256), FWD_LDS, (hipStream_t)stream, qkv, O, lse2, (int)T,
                       (int)nh, scale, dc);
  else
    hipLaunchKernelGGL(attn32_long_fwd_k<false>, grid, dim3(256), FWD_LDS, (hipStream_t)stream, qkv, O, lse2, (int)T,
                       (int)nh, scale, dc);
  B2P_CHECK_LAUNCH();
  return 0;
}

extern "C" int b2p_attn32_long_bwd(const float* qkv, const float* dO, const float* lse2, float* delta_ws, float* dqkv,
                                   int64_t B, int64_t T, int64_t nh, int64_t dh, float scale, float drop_p,
                                   uint64_t drop_seed, b2p_stream_t stream) {
  B2P_CHECK_ARG(qkv && dO && lse2 && delta_ws && dqkv, "attn32_long_bwd: NULL pointer");
  B2P_CHECK_ARG(aligned16(qkv) && aligned16(dO) && aligned16(dqkv),
                "attn32_long_bwd: qkv, dO and dqkv must be 16-byte aligned");
  if (long_args("attn32_long_bwd", B, T, nh, dh, drop_p)) return 1;
  if (B <= 0) return 0;
  if (init_attrs()) return 2;
  const dim3 grid((unsigned)(B * nh * ((T + BLK - 1) / BLK)));
  const DropCfg dc = drop_cfg(drop_p, drop_seed);
  hipStream_t st = (hipStream_t)stream;
  if (drop_p > 0.f) {
    hipLaunchKernelGGL(attn32_long_bwd_dq_k<true>, grid, dim3(256), FWD_LDS, st, qkv, dO, lse2, delta_ws, dqkv, (int)T,
                       (int)nh, scale, dc);
    hipLaunchKernelGGL(attn32_long_bwd_dkv_k<true>, grid, dim3(256), LONG_DKV_LDS, st, qkv, dO, lse2, delta_ws, dqkv,
                       (int)T, (int)nh, scale, dc);
  } else {
    hipLaunchKernelGGL(attn32_long_bwd_dq_k<false>, grid, dim3(256), FWD_LDS, st, qkv, dO, lse2, delta_ws, dqkv, (int)T,
                       (int)nh, scale, dc);
    hipLaunchKernelGGL(attn32_long_bwd_dkv_k<false>, grid, dim3(256), LONG_DKV_LDS, st, qkv, dO, lse2, delta_ws, dqkv,
                       (int)T, (int)nh, scale, dc);
  }
  B2P_CHECK_LAUNCH();
  return 0;
}
