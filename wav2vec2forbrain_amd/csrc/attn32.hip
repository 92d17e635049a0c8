// Fused exact-fp32 self-attention (forward + backward) for the w2v / Conformer encoder layers where the
// operands are fp32 (the bf16x3 precision mode by default, the fp32 mode on request: functional.ATTN32_MODES): softmax(Q K^T * scale) -> dropout -> @ V, no mask (reference: eager_attention_forward
// behind HF Wav2Vec2Attention; the Conformer's rotary self-attention core,
// w2v_conformer_custom_feat_extractor.py:79-112). Every product runs on v_mfma_f32_16x16x4_f32 (fp32 operands,
// fp32 accumulate: bitwise an fmaf chain), so nothing is rounded to 16 bits anywhere.
//
// One kernel family for head size 64 and T' <= 512. One (batch, head)'s K and V (backward: Q and dO) are staged
// as fp32 images of 256 rows, 2 x 64 KB of LDS, so the scores never touch HBM (the unfused path runs 6 batched
// GEMMs and 2 softmax kernels per layer over (B, heads, T', T') fp32 tensors and saves two of them for the
// backward). NC = 1 chunk of 256 rows is the 256 class (T' <= 256, b2p_attn32_fwd / _bwd); NC = 2 chunks, staged
// one after the other into the same two images, is the long class (257 <= T' <= 512, b2p_attn32_long_fwd /
// _bwd). The work split is csrc/attn16.hip's:
//   fwd   (b, h, 128-query block), attn32_fwd_k<NC>: S^T = K Q^T (keys in registers, query on the lane),
//         in-register softmax, O^T = V^T P^T. Saves lse2[b][h][q] = max + log2(sum) in the log2 domain. One
//         chunk: P is normalised before the product. Two chunks: online softmax, normalised at the store.
//   dQ    (b, h, 128-query block, launched first): S^T, dP^T recomputed from lse2 and normalised by their own
//         row sum; delta = sum_key P_d dP_d from those same values; both row constants go to delta_ws
//         ([2][B][nh][T]: delta, 1 / row sum); dQ^T += K^T dS^T. Two bodies: attn32_bwd_dq_k keeps a row's 256
//         P and dP in registers and sweeps once, attn32_long_bwd_dq_k sweeps its two chunks twice.
//   dK/dV (b, h, 128-key block), attn32_bwd_dkv_k<NC>: S, dP = dO V^T with the key on the lane; dV^T += dO^T P_d
//         and dK^T += Q^T dS with the dQ pass's delta.
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
constexpr int TMAX = 256;    // rows of an image: the keys / queries of one staged chunk
constexpr int TLONG = 512;   // keys / queries of one (batch, head) in the long class (two chunks)
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
// Stage rows [r0, r0 + 256) of a head slice (64 fp32 at column `col` of a row-major [B*T][ld] matrix) into an
// LDS image; rows >= T are zero. 256 threads, 16 chunks of 16 B each. SKIP leaves the 32-row tile pairs that lie
// wholly at or above T unwritten (T' = 313: 6 of the second chunk's 8).
// Invariant: every LDS tile a kernel reads was written by this launch (LDS is not cleared between launches,
// and a masked probability of 0 times a stale NaN is a NaN). Which tiles each kernel reads:
//   attn32_fwd_k<1>, attn32_bwd_dq_k  all 16 tiles of both images, unconditionally             -> SKIP = false
//   attn32_fwd_k<2>                   K tile pairs (kt, kt + 1) and V tiles kt with kt * 16 < Tc -> SKIP = true
//   attn32_long_bwd_dq_k              tiles kt < ceil(Tc / 16)                                  -> SKIP = true
//   attn32_bwd_dkv_k<NC>              tiles qt < ceil(Tc / 16)                                  -> SKIP = NC > 1
// with Tc = T - r0 the chunk's rows below T: each of those tiles lies in a pair whose first row is below T.
// The one-chunk dK/dV kernel could skip as well and does not: the branch around each pair's global loads cost
// the 256 class's backward 0.6 % at T' = 249, where nothing is skipped (profiles/r14a_attn32_refactor_parity.txt).
template <bool SKIP>
__device__ __forceinline__ void stage(char* img, const float* base, int64_t row0, int r0, int T, int64_t ld, int col,
                                      int tid) {
#pragma unroll
  for (int k = 0; k < TMAX / 16; ++k) {
    const int idx = tid + 256 * k;
    const int r = idx >> 4, c = idx & 15;
    if (!SKIP || r0 + (r & ~31) < T) {
      float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
      if (r0 + r < T) v = *reinterpret_cast<const float4*>(base + (row0 + r0 + r) * ld + col + 4 * c);
      *reinterpret_cast<float4*>(img + r * 256 + ((c ^ (r & 15)) << 4)) = v;
    }
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

// What every kernel of the family derives from its block and thread index: one workgroup of 4 waves per
// (batch, head, 128-row block); wave w runs the block's 16-row tiles w and w + 4.
struct Ctx {
  int tid, w, lr, g;        // thread, wave, lane & 15, lane >> 4
  int bh, b, h, blk;        // b * nh + h, its parts, the 128-row block of the head
  int D, TP;                // nh * 64; T rounded up to even (the dropout index's row stride)
  int64_t ld, row0, nrows;  // 3 * D; b * T; B * nh * T (a plane of delta_ws)
  int ro[4], co[4][4];      // row_off / col_off of this lane
  float c2;                 // scale * log2(e)
  uint64_t seed;            // the launch's effective dropout seed (b2p_seed_eff)
  uint32_t k32, thr16;      // b2p_hash key of that seed, 16-bit keep threshold
};
// Fills cx. Returns false when the LayerDrop gate is closed: the caller zero-fills its outputs from the index
// fields and returns; nothing but the gate has been read then, and the seed fields are not set.
__device__ __forceinline__ bool make_ctx(Ctx& cx, int T, int nh, float scale, const DropCfg& dc) {
  const int nblk = (T + BLK - 1) / BLK;
  cx.bh = blockIdx.x / nblk;
  cx.blk = blockIdx.x - cx.bh * nblk;
  cx.b = cx.bh / nh;
  cx.h = cx.bh - cx.b * nh;
  cx.D = nh * DH;
  cx.ld = 3 * (int64_t)cx.D;
  cx.tid = threadIdx.x;
  cx.w = cx.tid >> 6;
  const int l = cx.tid & 63;
  cx.lr = l & 15;
  cx.g = l >> 4;
  cx.row0 = (int64_t)cx.b * T;
  cx.nrows = (int64_t)(gridDim.x / nblk) * T;
  if (b2p_gated_off(dc.gate)) return false;
  cx.seed = b2p_seed_eff(dc.seed, dc.epoch);
#pragma unroll
  for (int j = 0; j < 4; ++j) cx.ro[j] = row_off(cx.lr, cx.g, j);
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) cx.co[i][dt] = col_off(cx.lr, cx.g, i, dt);
  cx.c2 = scale * LOG2E;
  cx.k32 = (uint32_t)cx.seed ^ b2p_mix32((uint32_t)(cx.seed >> 32) + 0x9E3779B9u);
  cx.thr16 = b2p_thr16(dc.thr);
  cx.TP = T + (T & 1);
  return true;
}

// ------------------------------------------------------------------------------------------ forward
// qkv [B*T][3*D] fp32 (q | k | v, head-major inside each); O [B*T][D]; lse2 [B][nh][T]. One workgroup per
// (batch, head, 128-query block): the 4 waves stage a chunk of K and V, then each wave runs its two query tiles
// over it. NC = 1: a row's 256 scores are all there, so P = exp2(s - max) / sum is formed before the PV product
// and a tile is stored as soon as it is done. NC = 2: each wave keeps its two tiles' running max, running sum and
// unnormalised O^T accumulators across the chunks (online softmax: a chunk rescales them by exp2(m_old - m_new))
// and divides by the sum at the store. The two roundings differ, and each class keeps its own.
template <int NC, bool DROP>
__global__ void __launch_bounds__(256) attn32_fwd_k(const float* __restrict__ qkv, float* __restrict__ O,
                                                    float* __restrict__ lse2, int T, int nh, float scale, DropCfg dc) {
  constexpr int NKT = TMAX / 16;
  constexpr bool ONE = NC == 1;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  Ctx cx;
  if (!make_ctx(cx, T, nh, scale, dc)) {   // LayerDrop: this replay skips the layer: O = 0, lse2 = 0 (finite)
    zero_block(O, cx.row0, cx.blk * BLK, T, cx.D, cx.h * DH, cx.tid);
    zero_rows(lse2, cx.bh, cx.blk * BLK, T, cx.tid);
    return;
  }
  const int g = cx.g, h = cx.h, D = cx.D;
  const int64_t ld = cx.ld, row0 = cx.row0;
  const float c2 = cx.c2;
  const char* Kimg = smem;
  const char* Vimg = smem + IMG_B;
  float mrun[2], lrun[2];
  f32x4 o[2][4];
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    mrun[j] = -INFINITY;
    lrun[j] = 0.f;
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) o[j][dt] = f32x4{0.f, 0.f, 0.f, 0.f};
  }
  for (int c = 0; c < NC; ++c) {
    const int r0 = c * TMAX;
    const int Tc = T - r0;   // keys of this chunk below T (every chunk holds one: NC = 2 has T > 256)
    if (c) __syncthreads();  // every wave is done with the previous chunk's images
    stage<!ONE>(smem, qkv, row0, r0, T, ld, D + h * DH, cx.tid);
    stage<!ONE>(smem + IMG_B, qkv, row0, r0, T, ld, 2 * D + h * DH, cx.tid);
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int qt = cx.blk * (BLK / 16) + cx.w + 4 * j;
      if (qt * 16 >= T) continue;
      const int q = qt * 16 + cx.lr;
      const bool qok = q < T;
      float qf[16];
      grow_frag(qkv + (row0 + (qok ? q : 0)) * ld + h * DH + 16 * g, qok, qf);
      // S^T of the chunk: tile kt = keys r0 + kt*16 + 4g + i (registers) x query q (lane); two tiles per pass
      // (independent chains)
      f32x4 s[NKT];
#pragma unroll
      for (int kt = 0; kt < NKT; kt += 2) {
        s[kt] = s[kt + 1] = f32x4{0.f, 0.f, 0.f, 0.f};
        if (ONE || kt * 16 < Tc) {
          float k0[16], k1[16];
          row_frag(Kimg + kt * TILE_B, cx.ro, k0);
          row_frag(Kimg + (kt + 1) * TILE_B, cx.ro, k1);
#pragma unroll
          for (int st = 0; st < 16; ++st) {
            s[kt] = mfma(k0[st], qf[st], s[kt]);
            s[kt + 1] = mfma(k1[st], qf[st], s[kt + 1]);
          }
        }
      }
      // row max of the raw scores (scale > 0 commutes with max); keys >= T -> -inf
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
      if constexpr (!ONE) m = fmaxf(m, mrun[j]);
      const float mc = m * c2;
      float alpha = 0.f;
      if constexpr (!ONE) {
        alpha = exp2_fast((mrun[j] - m) * c2);   // first chunk: exp2(-inf) = 0 over zeros
        mrun[j] = m;
      }
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
      float inv = 1.f;
      if constexpr (ONE) {
        inv = 1.f / sum;
      } else {
        lrun[j] = fmaf(lrun[j], alpha, sum);
#pragma unroll
        for (int dt = 0; dt < 4; ++dt)
#pragma unroll
          for (int i = 0; i < 4; ++i) o[j][dt][i] *= alpha;
      }
      const uint32_t rowlo =
          ((uint32_t)cx.bh * (uint32_t)T + (uint32_t)(qok ? q : 0)) * (uint32_t)cx.TP + (uint32_t)r0;
      // O^T (d x q) += V_c^T (d x keys) . P_d^T (keys x q): step (kt, i) sums keys kt*16 + 4g' + i, g' = 0..3
#pragma unroll
      for (int kt = 0; kt < NKT; ++kt) {
        if (!ONE && kt * 16 >= Tc) continue;
        const uint32_t kb = DROP ? keep4_bits(rowlo + (uint32_t)(kt * 16 + 4 * g), cx.k32, cx.thr16) : 0xFu;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          float pv = s[kt][i];
          if constexpr (ONE) pv *= inv;
          if constexpr (DROP) pv = ((kb >> i) & 1u) ? pv * dc.scale : 0.f;
#pragma unroll
          for (int dt = 0; dt < 4; ++dt)
            o[j][dt] = mfma(*reinterpret_cast<const float*>(Vimg + kt * TILE_B + cx.co[i][dt]), pv, o[j][dt]);
        }
      }
      if constexpr (ONE) {
        if (qok) {
          float* orow = O + (row0 + q) * D + h * DH + 4 * g;
#pragma unroll
          for (int dt = 0; dt < 4; ++dt)
            *reinterpret_cast<float4*>(orow + dt * 16) = make_float4(o[j][dt][0], o[j][dt][1], o[j][dt][2], o[j][dt][3]);
          if (g == 0) lse2[(int64_t)cx.bh * T + q] = mc + __log2f(sum);
        }
      }
    }
  }
  if constexpr (!ONE) {
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int q = (cx.blk * (BLK / 16) + cx.w + 4 * j) * 16 + cx.lr;
      if (q < T) {
        const float inv = 1.f / lrun[j];
        float* orow = O + (row0 + q) * D + h * DH + 4 * g;
#pragma unroll
        for (int dt = 0; dt < 4; ++dt)
          *reinterpret_cast<float4*>(orow + dt * 16) =
              make_float4(o[j][dt][0] * inv, o[j][dt][1] * inv, o[j][dt][2] * inv, o[j][dt][3] * inv);
        if (g == 0) lse2[(int64_t)cx.bh * T + q] = fmaf(mrun[j], c2, __log2f(lrun[j]));
      }
    }
  }
}

// --------------------------------------------------------------------------------------- backward dQ
// The pieces the two dQ kernels share.
// One query tile's visit of key tile kt of the staged chunk: S^T and dP^T tiles, P = exp2(s - lse2),
// dP_d = dP * keep. Keys at or above Tc (the chunk's keys below T) are masked; rows q >= T need no mask (a
// lane's dS only reaches its own, unstored dQ row). rowlo: the dropout index of the chunk's first key. SUMS: dl
// and rs also take the lane's parts of sum_key P dP_d and of the row sum.
template <bool DROP, bool SUMS>
__device__ __forceinline__ void dq_scores(const char* Kimg, const char* Vimg, const Ctx& cx, const float (&qf)[16],
                                          const float (&df)[16], float ls, uint32_t rowlo, int kt, int Tc,
                                          float dscale, f32x4& P, f32x4& PD, float& dl, float& rs) {
  float kf[16], vf[16];
  row_frag(Kimg + kt * TILE_B, cx.ro, kf);
  row_frag(Vimg + kt * TILE_B, cx.ro, vf);
  f32x4 sv = f32x4{0.f, 0.f, 0.f, 0.f}, dp = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int st = 0; st < 16; ++st) {
    sv = mfma(kf[st], qf[st], sv);
    dp = mfma(vf[st], df[st], dp);
  }
  const uint32_t kb = DROP ? keep4_bits(rowlo + (uint32_t)(kt * 16 + 4 * cx.g), cx.k32, cx.thr16) : 0xFu;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const bool ok = kt * 16 + 4 * cx.g + i < Tc;
    const float p = ok ? exp2_fast(fmaf(sv[i], cx.c2, -ls)) : 0.f;
    float pd = dp[i];
    if constexpr (DROP) pd = ((kb >> i) & 1u) ? pd * dscale : 0.f;
    pd = ok ? pd : 0.f;
    P[i] = p;
    PD[i] = pd;
    if constexpr (SUMS) {
      dl += p * pd;
      rs += p;
    }
  }
}
// dS = P (dP_d - dl) with the finished dl, dQ^T += K_c^T dS^T over key tile kt
__device__ __forceinline__ void dq_accum(const char* Kimg, const Ctx& cx, int kt, const f32x4& P, const f32x4& PD,
                                         float dl, f32x4 (&dq)[4]) {
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const float ds = P[i] * (PD[i] - dl);
#pragma unroll
    for (int dt = 0; dt < 4; ++dt)
      dq[dt] = mfma(*reinterpret_cast<const float*>(Kimg + kt * TILE_B + cx.co[i][dt]), ds, dq[dt]);
  }
}
// One query tile's sweep over the staged chunk's key tiles below T (the long class; the 256 class unrolls its own
// 16 tiles around the same pieces). SECOND = false: the row constants' parts. SECOND = true: dQ^T.
template <bool DROP, bool SECOND>
__device__ __forceinline__ void dq_sweep(const char* Kimg, const char* Vimg, const Ctx& cx, const float (&qf)[16],
                                         const float (&df)[16], float ls, uint32_t rowlo, int Tc, float dscale,
                                         float& dl, float& rs, f32x4 (&dq)[4]) {
  const int nkt = Tc < TMAX ? (Tc + 15) >> 4 : TMAX / 16;
  for (int kt = 0; kt < nkt; ++kt) {
    f32x4 P, PD;
    dq_scores<DROP, !SECOND>(Kimg, Vimg, cx, qf, df, ls, rowlo, kt, Tc, dscale, P, PD, dl, rs);
    if constexpr (SECOND) dq_accum(Kimg, cx, kt, P, PD, dl, dq);
  }
}
// The row constants from the lanes' parts over all keys; returns 1 / row sum, dl becomes delta.
// The recomputed row p = exp2(s - lse2) sums to rs = 1 + e, |e| up to ~6e-7: lse2 is one fp32 near 8 (its
// ulp there is 9.5e-7 in the log2 domain) and the v_log_f32 / v_exp_f32 results carry an ulp each. A
// row-coherent error of that size in P is ~6x the rounding noise of the unfused path's stored P, and the
// full fine-tune's Adam trajectory (updates ~lr * sign(g)) follows it: measured 3.6e-5 / 2.0e-4 at steps
// 2 / 3 of conformer_large_ft_bs8 in fp32 mode against 5.4e-6 / 6.4e-5 unfused. So both backward kernels
// normalise p by the row sum the dQ kernel forms: 1 / rs goes to the second plane of delta_ws for dK/dV,
// delta is the normalised rows' (sum_key dS = 0 holds to rounding), dQ's own row is scaled at the store.
__device__ __forceinline__ float dq_row_consts(const Ctx& cx, bool qok, int64_t rowc, float& dl, float rs,
                                               float* delta) {
  dl += __shfl_xor(dl, 16, 64);
  dl += __shfl_xor(dl, 32, 64);
  rs += __shfl_xor(rs, 16, 64);
  rs += __shfl_xor(rs, 32, 64);
  const float irs = 1.f / rs;
  dl *= irs;
  if (qok && cx.g == 0) {
    delta[rowc] = dl;
    delta[cx.nrows + rowc] = irs;
  }
  return irs;
}
__device__ __forceinline__ void dq_store(float* dqkv, const Ctx& cx, int q, const f32x4 (&dq)[4], float qs) {
  float* r = dqkv + (cx.row0 + q) * cx.ld + cx.h * DH + 4 * cx.g;
#pragma unroll
  for (int dt = 0; dt < 4; ++dt)
    *reinterpret_cast<float4*>(r + dt * 16) =
        make_float4(dq[dt][0] * qs, dq[dt][1] * qs, dq[dt][2] * qs, dq[dt][3] * qs);
}

// Both dQ kernels run BEFORE the dK/dV kernel: delta[q] = sum_key P_d dP_d is formed here from the very P and
// dP the kernel recomputes, so sum_key dS = 0 holds to fp32 rounding. One workgroup per (batch, head, 128
// queries). The 256 class stages K and V once: pass 1 keeps a row's P and dP*keep in registers (dq_scores of
// all 16 tiles), pass 2 forms dS and dQ^T from them (dq_accum) without a second product.
template <bool DROP>
__global__ void __launch_bounds__(256) attn32_bwd_dq_k(const float* __restrict__ qkv, const float* __restrict__ dO,
                                                       const float* __restrict__ lse2, float* __restrict__ delta,
                                                       float* __restrict__ dqkv, int T, int nh, float scale,
                                                       DropCfg dc) {
  constexpr int NKT = TMAX / 16;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  Ctx cx;
  if (!make_ctx(cx, T, nh, scale, dc)) {   // LayerDrop: zero dQ and delta
    zero_block(dqkv, cx.row0, cx.blk * BLK, T, cx.ld, cx.h * DH, cx.tid);
    zero_rows(delta, cx.bh, cx.blk * BLK, T, cx.tid);
    zero_rows(delta + cx.nrows, cx.bh, cx.blk * BLK, T, cx.tid);
    return;
  }
  stage<false>(smem, qkv, cx.row0, 0, T, cx.ld, cx.D + cx.h * DH, cx.tid);
  stage<false>(smem + IMG_B, qkv, cx.row0, 0, T, cx.ld, 2 * cx.D + cx.h * DH, cx.tid);
  __syncthreads();
  const char* Kimg = smem;
  const char* Vimg = smem + IMG_B;
  const int qt0 = cx.blk * (BLK / 16) + cx.w;
  for (int qt = qt0; qt < (cx.blk + 1) * (BLK / 16) && qt * 16 < T; qt += 4) {
    const int q = qt * 16 + cx.lr;
    const bool qok = q < T;
    float qf[16], df[16];
    grow_frag(qkv + (cx.row0 + (qok ? q : 0)) * cx.ld + cx.h * DH + 16 * cx.g, qok, qf);
    grow_frag(dO + (cx.row0 + (qok ? q : 0)) * cx.D + cx.h * DH + 16 * cx.g, qok, df);
    const int64_t rowc = (int64_t)cx.bh * T + (qok ? q : 0);
    const float ls = qok ? lse2[rowc] : 0.f;
    const uint32_t rowlo = (uint32_t)rowc * (uint32_t)cx.TP;
    f32x4 P[NKT], PD[NKT];
    float dl = 0.f, rs = 0.f;
#pragma unroll
    for (int kt = 0; kt < NKT; ++kt)
      dq_scores<DROP, true>(Kimg, Vimg, cx, qf, df, ls, rowlo, kt, T, dc.scale, P[kt], PD[kt], dl, rs);
    const float irs = dq_row_consts(cx, qok, rowc, dl, rs, delta);
    f32x4 dq[4];
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) dq[dt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int kt = 0; kt < NKT; ++kt) dq_accum(Kimg, cx, kt, P[kt], PD[kt], dl, dq);
    if (qok) dq_store(dqkv, cx, q, dq, scale * irs);
  }
}

// The long class. delta over all keys is needed before any dS and a row's 512 P and dP do not fit in registers
// beside a second tile's, so the chunks are swept twice: (chunk 0, chunk 1) for the row constants, then (chunk
// 1, still staged, chunk 0) for dQ: three stagings, and S^T / dP^T computed twice (dq_scores in both sweeps).
template <bool DROP>
__global__ void __launch_bounds__(256) attn32_long_bwd_dq_k(const float* __restrict__ qkv,
                                                            const float* __restrict__ dO,
                                                            const float* __restrict__ lse2, float* __restrict__ delta,
                                                            float* __restrict__ dqkv, int T, int nh, float scale,
                                                            DropCfg dc) {
  constexpr int NC = TLONG / TMAX;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  Ctx cx;
  if (!make_ctx(cx, T, nh, scale, dc)) {   // LayerDrop: zero dQ and delta
    zero_block(dqkv, cx.row0, cx.blk * BLK, T, cx.ld, cx.h * DH, cx.tid);
    zero_rows(delta, cx.bh, cx.blk * BLK, T, cx.tid);
    zero_rows(delta + cx.nrows, cx.bh, cx.blk * BLK, T, cx.tid);
    return;
  }
  const char* Kimg = smem;
  const char* Vimg = smem + IMG_B;
  float dl[2] = {0.f, 0.f}, rs[2] = {0.f, 0.f}, irs[2] = {0.f, 0.f};
  f32x4 dq[2][4];
#pragma unroll
  for (int j = 0; j < 2; ++j)
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) dq[j][dt] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int ph = 0; ph < 2 * NC; ++ph) {   // (sweep, chunk): (0, 0) (0, 1) (1, 1) (1, 0)
    const int c = (ph == 1 || ph == 2) ? 1 : 0;
    const int r0 = c * TMAX;
    if (ph != 2) {
      if (ph) __syncthreads();   // every wave is done with the staged chunk
      stage<true>(smem, qkv, cx.row0, r0, T, cx.ld, cx.D + cx.h * DH, cx.tid);
      stage<true>(smem + IMG_B, qkv, cx.row0, r0, T, cx.ld, 2 * cx.D + cx.h * DH, cx.tid);
      __syncthreads();
    }
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int qt = cx.blk * (BLK / 16) + cx.w + 4 * j;
      if (qt * 16 >= T) continue;
      const int q = qt * 16 + cx.lr;
      const bool qok = q < T;
      float qf[16], df[16];
      grow_frag(qkv + (cx.row0 + (qok ? q : 0)) * cx.ld + cx.h * DH + 16 * cx.g, qok, qf);
      grow_frag(dO + (cx.row0 + (qok ? q : 0)) * cx.D + cx.h * DH + 16 * cx.g, qok, df);
      const int64_t rowc = (int64_t)cx.bh * T + (qok ? q : 0);
      const float ls = qok ? lse2[rowc] : 0.f;
      const uint32_t rowlo = (uint32_t)rowc * (uint32_t)cx.TP + (uint32_t)r0;
      if (ph < 2) {
        dq_sweep<DROP, false>(Kimg, Vimg, cx, qf, df, ls, rowlo, T - r0, dc.scale, dl[j], rs[j], dq[j]);
        if (ph == 1) irs[j] = dq_row_consts(cx, qok, rowc, dl[j], rs[j], delta);   // both chunks seen
      } else {
        dq_sweep<DROP, true>(Kimg, Vimg, cx, qf, df, ls, rowlo, T - r0, dc.scale, dl[j], rs[j], dq[j]);
      }
    }
  }
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int q = (cx.blk * (BLK / 16) + cx.w + 4 * j) * 16 + cx.lr;
    if (q < T) dq_store(dqkv, cx, q, dq[j], scale * irs[j]);
  }
}

// ------------------------------------------------------------------------------------ backward dK dV
// delta_ws [2][B][nh][T] from the dQ kernel (delta, 1 / row sum); writes dK, dV into dqkv columns [D + h*64, ...)
// and [2D + h*64, ...). One workgroup per (batch, head, 128 keys), the key on the lane; Q and dO are staged in NC
// chunks, a wave's key tiles w and w + 4 accumulate dK^T and dV^T over them. The row constants of all T queries
// (lse2 and the dQ kernel's two planes) sit in LDS beside the images.
template <int NC, bool DROP>
__global__ void __launch_bounds__(256) attn32_bwd_dkv_k(const float* __restrict__ qkv, const float* __restrict__ dO,
                                                        const float* __restrict__ lse2, const float* __restrict__ delta,
                                                        float* __restrict__ dqkv, int T, int nh, float scale,
                                                        DropCfg dc) {
  constexpr int TCLS = NC * TMAX;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* lse_s = reinterpret_cast<float*>(smem + 2 * IMG_B);
  float* del_s = lse_s + TCLS;
  float* irs_s = del_s + TCLS;
  Ctx cx;
  if (!make_ctx(cx, T, nh, scale, dc)) {   // LayerDrop: zero dK, dV
    zero_block(dqkv, cx.row0, cx.blk * BLK, T, cx.ld, cx.D + cx.h * DH, cx.tid);
    zero_block(dqkv, cx.row0, cx.blk * BLK, T, cx.ld, 2 * cx.D + cx.h * DH, cx.tid);
    return;
  }
  const int g = cx.g, h = cx.h, D = cx.D;
  const int64_t ld = cx.ld, row0 = cx.row0;
  for (int qq = cx.tid; qq < TCLS; qq += 256) {
    const int64_t o = (int64_t)cx.bh * T + qq;
    lse_s[qq] = qq < T ? lse2[o] : 0.f;
    del_s[qq] = qq < T ? delta[o] : 0.f;
    irs_s[qq] = qq < T ? delta[cx.nrows + o] : 0.f;
  }
  const char* Qimg = smem;
  const char* dOimg = smem + IMG_B;
  // NC = 1: a wave runs its two key tiles one after the other through one set of accumulators (a runtime loop:
  // unrolled over both sets it ran the 256 class's backward 0.4 % slower, profiles/r14a_attn32_refactor_parity.txt).
  // NC = 2: both tiles' sets live across the chunks (the loop over the tiles is unrolled).
  constexpr int NACC = NC == 1 ? 1 : 2;
  f32x4 dv[NACC][4], dk[NACC][4];
#pragma unroll
  for (int a = 0; a < NACC; ++a)
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) dv[a][dt] = dk[a][dt] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int c = 0; c < NC; ++c) {   // a key tile is stored as soon as its last chunk is done
    const int r0 = c * TMAX;
    if (c) __syncthreads();   // every wave is done with the previous chunk's images
    stage<(NC > 1)>(smem, qkv, row0, r0, T, ld, h * DH, cx.tid);
    stage<(NC > 1)>(smem + IMG_B, dO, row0, r0, T, D, h * DH, cx.tid);
    __syncthreads();
    const int nqt = T - r0 < TMAX ? (T - r0 + 15) >> 4 : TMAX / 16;
#pragma unroll(NACC)
    for (int j = 0; j < 2; ++j) {
      const int kt = cx.blk * (BLK / 16) + cx.w + 4 * j;
      if (kt * 16 >= T) continue;
      const int a = NC == 1 ? 0 : j;
      if constexpr (NC == 1) {
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) dv[0][dt] = dk[0][dt] = f32x4{0.f, 0.f, 0.f, 0.f};
      }
      const int key = kt * 16 + cx.lr;
      const bool kok = key < T;
      float kf[16], vf[16];
      grow_frag(qkv + (row0 + (kok ? key : 0)) * ld + D + h * DH + 16 * g, kok, kf);
      grow_frag(qkv + (row0 + (kok ? key : 0)) * ld + 2 * D + h * DH + 16 * g, kok, vf);
      for (int qt = 0; qt < nqt; ++qt) {
        const char* Qt = Qimg + qt * TILE_B;
        const char* dOt = dOimg + qt * TILE_B;
        float qf[16], of[16];
        row_frag(Qt, cx.ro, qf);
        row_frag(dOt, cx.ro, of);
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
          const float p = q0 + i < T ? exp2_fast(fmaf(sv[i], cx.c2, -lsv[i])) * irv[i] : 0.f;   // over the row sum (dQ pass)
          float ksc = 1.f;
          if constexpr (DROP)
            ksc = b2p_keep(cx.seed, ((uint64_t)cx.bh * T + (uint64_t)(q0 + i)) * (uint64_t)cx.TP + (uint64_t)key, dc.thr)
                      ? dc.scale : 0.f;
          pd[i] = p * ksc;
          ds[i] = p * (dp[i] * ksc - dlv[i]);
        }
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int dt = 0; dt < 4; ++dt) {
            dv[a][dt] = mfma(*reinterpret_cast<const float*>(dOt + cx.co[i][dt]), pd[i], dv[a][dt]);
            dk[a][dt] = mfma(*reinterpret_cast<const float*>(Qt + cx.co[i][dt]), ds[i], dk[a][dt]);
          }
      }
      if (c == NC - 1 && kok) {
        float* r = dqkv + (row0 + key) * ld + h * DH + 4 * g;
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) {
          *reinterpret_cast<float4*>(r + D + dt * 16) =
              make_float4(dk[a][dt][0] * scale, dk[a][dt][1] * scale, dk[a][dt][2] * scale, dk[a][dt][3] * scale);
          *reinterpret_cast<float4*>(r + 2 * D + dt * 16) =
              make_float4(dv[a][dt][0], dv[a][dt][1], dv[a][dt][2], dv[a][dt][3]);
        }
      }
    }
  }
}

// ------------------------------------------------------------------------------------------------ host
// The two shape classes: index 0 is the 256 class (one chunk), index 1 the long class (two chunks).
struct Cls {
  const char* fwd;
  const char* bwd;
  int64_t tmin, tmax;
  const char* range;
};
const Cls CLS[2] = {{"attn32_fwd", "attn32_bwd", 1, TMAX, "1 <= T <= 256"},
                    {"attn32_long_fwd", "attn32_long_bwd", TMAX + 1, TLONG,
                     "257 <= T <= 512 (b2p_attn32_fwd / _bwd serve T <= 256)"}};
using FwdK = void (*)(const float*, float*, float*, int, int, float, DropCfg);
using DqK = void (*)(const float*, const float*, const float*, float*, float*, int, int, float, DropCfg);
using DkvK = void (*)(const float*, const float*, const float*, const float*, float*, int, int, float, DropCfg);
// [class][drop_p > 0]
const FwdK FWD_K[2][2] = {{attn32_fwd_k<1, false>, attn32_fwd_k<1, true>}, {attn32_fwd_k<2, false>, attn32_fwd_k<2, true>}};
const DqK DQ_K[2][2] = {{attn32_bwd_dq_k<false>, attn32_bwd_dq_k<true>},
                        {attn32_long_bwd_dq_k<false>, attn32_long_bwd_dq_k<true>}};
const DkvK DKV_K[2][2] = {{attn32_bwd_dkv_k<1, false>, attn32_bwd_dkv_k<1, true>},
                          {attn32_bwd_dkv_k<2, false>, attn32_bwd_dkv_k<2, true>}};
constexpr size_t IMG2_LDS = 2 * IMG_B;   // forward and dQ: the two images
constexpr size_t dkv_lds(int cls) { return 2 * IMG_B + 3 * (size_t)(cls + 1) * TMAX * 4; }   // + the row constants

int init_attrs() {
  static int done = -1;
  if (done >= 0) return done;
  for (int cls = 0; cls < 2; ++cls)
    for (int drop = 0; drop < 2; ++drop) {
      const struct { const void* k; size_t lds; } tab[3] = {{(const void*)FWD_K[cls][drop], IMG2_LDS},
                                                           {(const void*)DQ_K[cls][drop], IMG2_LDS},
                                                           {(const void*)DKV_K[cls][drop], dkv_lds(cls)}};
      for (const auto& e : tab)
        B2P_CHECK_HIP(hipFuncSetAttribute(e.k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)e.lds));
    }
  done = 0;
  return done;
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
bool aligned16(const void* p) { return ((uintptr_t)p & 15u) == 0; }
bool in_class(int cls, int64_t T, int64_t dh) { return dh == DH && T >= CLS[cls].tmin && T <= CLS[cls].tmax; }

// The checks every call shares, both directions and both classes (1: rejected, the error is set).
int check_args(const char* what, int cls, bool nonnull, bool al16, int64_t B, int64_t T, int64_t nh, int64_t dh,
               float drop_p) {
  B2P_CHECK_ARG(nonnull, "%s: NULL pointer", what);
  B2P_CHECK_ARG(al16, "%s: qkv, O, dO and dqkv must be 16-byte aligned", what);
  B2P_CHECK_ARG(dh == DH, "%s: needs head size 64", what);
  B2P_CHECK_ARG(in_class(cls, T, dh), "%s: needs %s", what, CLS[cls].range);
  B2P_CHECK_ARG(nh > 0, "%s: needs heads > 0", what);
  B2P_CHECK_ARG(drop_p >= 0.f && drop_p < 1.f, "%s: needs 0 <= drop_p < 1", what);
  B2P_CHECK_ARG(B <= 0 || B * nh * T * (T + (T & 1)) < (1ll << 32), "%s: B * heads * T * T must stay below 2^32 "
                "(32-bit dropout element index)", what);
  return 0;
}

int launch_fwd(int cls, const float* qkv, float* O, float* lse2, int64_t B, int64_t T, int64_t nh, int64_t dh,
               float scale, float drop_p, uint64_t drop_seed, b2p_stream_t stream) {
  if (check_args(CLS[cls].fwd, cls, qkv && O && lse2, aligned16(qkv) && aligned16(O), B, T, nh, dh, drop_p)) return 1;
  if (B <= 0) return 0;
  if (init_attrs()) return 2;
  const dim3 grid((unsigned)(B * nh * ((T + BLK - 1) / BLK)));
  hipLaunchKernelGGL(FWD_K[cls][drop_p > 0.f], grid, dim3(256), IMG2_LDS, (hipStream_t)stream, qkv, O, lse2, (int)T,
                     (int)nh, scale, drop_cfg(drop_p, drop_seed));
  B2P_CHECK_LAUNCH();
  return 0;
}

int launch_bwd(int cls, const float* qkv, const float* dO, const float* lse2, float* delta_ws, float* dqkv, int64_t B,
               int64_t T, int64_t nh, int64_t dh, float scale, float drop_p, uint64_t drop_seed, b2p_stream_t stream) {
  if (check_args(CLS[cls].bwd, cls, qkv && dO && lse2 && delta_ws && dqkv,
                 aligned16(qkv) && aligned16(dO) && aligned16(dqkv), B, T, nh, dh, drop_p))
    return 1;
  if (B <= 0) return 0;
  if (init_attrs()) return 2;
  const dim3 grid((unsigned)(B * nh * ((T + BLK - 1) / BLK)));
  const DropCfg dc = drop_cfg(drop_p, drop_seed);
  const int drop = drop_p > 0.f;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(DQ_K[cls][drop], grid, dim3(256), IMG2_LDS, st, qkv, dO, lse2, delta_ws, dqkv, (int)T, (int)nh,
                     scale, dc);
  hipLaunchKernelGGL(DKV_K[cls][drop], grid, dim3(256), dkv_lds(cls), st, qkv, dO, lse2, (const float*)delta_ws, dqkv,
                     (int)T, (int)nh, scale, dc);
  B2P_CHECK_LAUNCH();
  return 0;
}
}  // namespace

extern "C" int b2p_attn32_supported(int64_t T, int64_t dh) { return in_class(0, T, dh) ? 1 : 0; }
extern "C" int b2p_attn32_long_supported(int64_t T, int64_t dh) { return in_class(1, T, dh) ? 1 : 0; }

extern "C" int b2p_attn32_fwd(const float* qkv, float* O, float* lse2, int64_t B, int64_t T, int64_t nh, int64_t dh,
                              float scale, float drop_p, uint64_t drop_seed, b2p_stream_t stream) {
  return launch_fwd(0, qkv, O, lse2, B, T, nh, dh, scale, drop_p, drop_seed, stream);
}
extern "C" int b2p_attn32_bwd(const float* qkv, const float* dO, const float* lse2, float* delta_ws, float* dqkv,
                              int64_t B, int64_t T, int64_t nh, int64_t dh, float scale, float drop_p,
                              uint64_t drop_seed, b2p_stream_t stream) {
  return launch_bwd(0, qkv, dO, lse2, delta_ws, dqkv, B, T, nh, dh, scale, drop_p, drop_seed, stream);
}
extern "C" int b2p_attn32_long_fwd(const float* qkv, float* O, float* lse2, int64_t B, int64_t T, int64_t nh,
                                   int64_t dh, float scale, float drop_p, uint64_t drop_seed, b2p_stream_t stream) {
  return launch_fwd(1, qkv, O, lse2, B, T, nh, dh, scale, drop_p, drop_seed, stream);
}
extern "C" int b2p_attn32_long_bwd(const float* qkv, const float* dO, const float* lse2, float* delta_ws, float* dqkv,
                                   int64_t B, int64_t T, int64_t nh, int64_t dh, float scale, float drop_p,
                                   uint64_t drop_seed, b2p_stream_t stream) {
  return launch_bwd(1, qkv, dO, lse2, delta_ws, dqkv, B, T, nh, dh, scale, drop_p, drop_seed, stream);
}
