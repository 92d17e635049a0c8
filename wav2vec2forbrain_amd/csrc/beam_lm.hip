// On-device CTC prefix beam search with shallow fusion of a word-level back-off n-gram language model:
// the decoding of the reference's test evaluator (pyctcdecode + KenLM through
// Wav2Vec2ProcessorWithLM, src/train/evaluator.py:148-154,189-210) with the LM read from a local ARPA
// file (wav2vec2forbrain_amd/util/ngram_lm.py builds the device image). The CTC part is csrc/beam.hip's
// search unchanged: candidate k = w*C + c, the stay / merge / suppress rules, the 64-bit prefix hash
// chain, the bitonic top-W, the history records. Added per beam: the trie node of the current word
// part (DEAD: no word has this prefix), its length, the last four word ids, the accumulated LM score.
//
// Scoring rule (float32 adds in the order written; LM values arrive multiplied by alpha):
//   word score, when a beam with a non-empty word part is extended by the delimiter:
//       delta = ((sum of back-offs + logp) + unk) + beta
//     by the usual back-off walk over (h_last k, w), k = order-1 .. 0; w = word_of(node), or <unk> with
//     unk = alpha * ln10 * unk_score_offset when the node is DEAD or ends no word;
//   delimiter after an empty word part: nothing is scored;
//   letter: node' = child(node, c) or DEAD; every non-blank, non-delimiter token is a letter;
//   partial-word penalty (ranking only): pen = node' == DEAD ? unk_score_offset * max(1, len'/6) : 0;
//   rank = (tot + acc') + pen replaces tot in the best-candidate maximum, the beam_prune_logp
//   threshold and the sort key;
//   end of sequence, for every live beam: a trailing word part is scored as a word, then with
//   score_boundary the score of </s> given the resulting history is added (the history then starts
//   as [<s>]); the beam with the best final rank (ties: lower slot) is read back.
// Restated in float32 by tests/beam_lm_restatement.py; parity against pyctcdecode itself is unpinned.
//
// One 256-thread workgroup per sample; W <= 128, C <= 64, order <= 5. The tables are open-addressing
// hash tables in global memory whose keys are 64-bit fingerprints the host verified to be distinct.
#include "common.h"
#include "../../include/b2p_hip.h"

namespace {

constexpr int BM_W = 128;
constexpr int BM_C = 64;
constexpr int BM_N = BM_W * BM_C;   // candidate slots (sorted bitonically)
constexpr int BM_H = 4;             // word ids of history kept per beam (order - 1 <= 4)
constexpr float NEG = -INFINITY;
constexpr int DEAD = -1;

struct LmImage {
  const uint64_t* trie_keys;
  const int32_t* trie_child;
  const int32_t* node_word;
  const uint64_t* ng_keys;
  const float2* ng_vals;   // (alpha * ln p, alpha * ln back-off)
  uint64_t trie_seed, ng_seed;
  uint32_t trie_mask, ng_mask;
  int order, unk_id, bos_id, eos_id;
  float beta, unk_scaled, unk_offset;
  int boundary;
};

__device__ __forceinline__ float lse2(float a, float b) {
  if (a == NEG) return b;
  if (b == NEG) return a;
  const float m = fmaxf(a, b);
  return m + log1pf(expf(-fabsf(a - b)));
}
__device__ __forceinline__ uint64_t hmix(uint64_t h, int c) { return (h ^ (uint64_t)(c + 1)) * 0x100000001B3ull; }
// float -> uint32 with the same order (for the descending-score sort key)
__device__ __forceinline__ uint32_t ord(float f) {
  const uint32_t u = __float_as_uint(f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
// one link of the fingerprint chain (util/ngram_lm.py fp_step): splitmix64's finaliser
__device__ __forceinline__ uint64_t fp_step(uint64_t h, int v) {
  uint64_t x = (h ^ (uint64_t)(uint32_t)(v + 1)) + 0x9E3779B97F4A7C15ull;
  x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
  x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
  return x ^ (x >> 31);
}

__device__ __forceinline__ int trie_child(const LmImage& L, int node, int c) {
  if (node == DEAD) return DEAD;
  const uint64_t f = fp_step(fp_step(L.trie_seed, node), c);
  uint32_t s = (uint32_t)f & L.trie_mask;
  for (uint32_t i = 0; i <= L.trie_mask; ++i) {   // load <= 0.5: ends at a hit or an empty slot
    const uint64_t k = L.trie_keys[s];
    if (k == f) return L.trie_child[s];
    if (k == 0) break;
    s = (s + 1) & L.trie_mask;
  }
  return DEAD;
}

__device__ __forceinline__ bool ng_find(const LmImage& L, uint64_t f, float2& v) {
  uint32_t s = (uint32_t)f & L.ng_mask;
  for (uint32_t i = 0; i <= L.ng_mask; ++i) {
    const uint64_t k = L.ng_keys[s];
    if (k == f) {
      v = L.ng_vals[s];
      return true;
    }
    if (k == 0) break;
    s = (s + 1) & L.ng_mask;
  }
  return false;
}

// sum of back-offs + logp of word w after the history h[0 .. BM_H-1] of beam slot (LDS, stride BM_W;
// most recent last, -1 = absent)
__device__ __forceinline__ float word_lm(const LmImage& L, const int (*h)[BM_W], int slot, int w) {
  int n = 0;
  while (n < L.order - 1 && h[BM_H - 1 - n][slot] >= 0) ++n;
  float bo = 0.f;
  for (int k = n; k >= 0; --k) {
    uint64_t f = L.ng_seed;
    for (int j = BM_H - k; j < BM_H; ++j) f = fp_step(f, h[j][slot]);
    float2 v;
    if (ng_find(L, fp_step(f, w), v)) return bo + v.x;
    if (k > 0 && ng_find(L, f, v)) bo = bo + v.y;
  }
  return bo;   // not reached: every word id has a unigram
}

__device__ __forceinline__ float partial_penalty(const LmImage& L, int node, int len) {
  return node == DEAD ? __fmul_rn(L.unk_offset, fmaxf(1.f, (float)len / 6.f)) : 0.f;
}

__global__ void __launch_bounds__(256) ctc_beam_lm_k(const float* __restrict__ logits, int T, int C,
                                                     const int32_t* __restrict__ lens, int W, int blank, int delim,
                                                     float token_min_logp, float prune_logp, const LmImage L,
                                                     int32_t* __restrict__ hist, int32_t* __restrict__ out_tok,
                                                     int32_t* __restrict__ out_len, float* __restrict__ out_ctc,
                                                     float* __restrict__ out_fused) {
  __shared__ float y[BM_C];
  __shared__ float pb[BM_W], pnb[BM_W];
  __shared__ uint64_t hs[BM_W], phs[BM_W];
  __shared__ int last[BM_W], blen[BM_W];
  __shared__ float cb[BM_N], cnb[BM_N];
  __shared__ uint64_t key[BM_N];
  __shared__ float sh_red[256];
  __shared__ int sh_arg;
  __shared__ float sh_best;
  // LM state of a beam: trie node and length of its word part, word history, accumulated score
  __shared__ int node[BM_W], wlen[BM_W], wh[BM_H][BM_W];
  __shared__ float acc[BM_W];
  // the word a beam's word part ends, and its score, if the delimiter follows (this frame)
  __shared__ float dscore[BM_W];
  __shared__ int dword[BM_W];
  // next-beam staging
  __shared__ float npb[BM_W], npnb[BM_W];
  __shared__ uint64_t nhs[BM_W], nphs[BM_W];
  __shared__ int nlast[BM_W], nlen[BM_W];
  __shared__ int nnode[BM_W], nwlen[BM_W], nwh[BM_H][BM_W];
  __shared__ float nacc[BM_W];

  const int b = blockIdx.x, tid = threadIdx.x;
  const int Tb = lens ? min(max(lens[b], 0), T) : T;
  const float* lg = logits + (int64_t)b * T * C;
  int32_t* hb = hist + (int64_t)b * T * W;
  const int N = W * C;
  int np2 = 1;
  while (np2 < N) np2 <<= 1;

  for (int w = tid; w < W; w += 256) {
    pb[w] = w == 0 ? 0.f : NEG;
    pnb[w] = NEG;
    hs[w] = 0xCBF29CE484222325ull;
    phs[w] = 0;
    last[w] = -1;
    blen[w] = 0;
    node[w] = 0;
    wlen[w] = 0;
    for (int j = 0; j < BM_H; ++j) wh[j][w] = -1;
    if (L.boundary) wh[BM_H - 1][w] = L.bos_id;
    acc[w] = 0.f;
  }
  __syncthreads();
  for (int t = 0; t < Tb; ++t) {
    // log-softmax of frame t (C <= 64: one wave) and its argmax
    if (tid < 64) {
      const float v = tid < C ? lg[(int64_t)t * C + tid] : NEG;
      float m = v;
      int am = tid < C ? tid : 1 << 30;
      for (int o = 32; o > 0; o >>= 1) {
        const float m2 = __shfl_xor(m, o, 64);
        const int a2 = __shfl_xor(am, o, 64);
        if (m2 > m || (m2 == m && a2 < am)) { m = m2; am = a2; }
      }
      float s = tid < C ? expf(v - m) : 0.f;
      for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
      if (tid < C) y[tid] = v - m - logf(s);
      if (tid == 0) sh_arg = am;
    }
    __syncthreads();
    const int arg = sh_arg;
    // candidates
    for (int k = tid; k < np2; k += 256) {
      float vb = NEG, vnb = NEG;
      if (k < N) {
        const int w = k / C, c = k - w * C;
        const float tot = lse2(pb[w], pnb[w]);
        const bool use = y[c] >= token_min_logp || c == arg;
        if (tot != NEG) {
          if (c == blank) {   // the stay candidate: blank path (if blank is used) + repeat path (if last is)
            if (use) vb = tot + y[blank];
            const int l = last[w];
            if (l >= 0 && (y[l] >= token_min_logp || l == arg)) vnb = pnb[w] + y[l];
          } else if (use) {
            vnb = (c == last[w] ? pb[w] : tot) + y[c];
          }
        }
      }
      cb[k] = vb;
      cnb[k] = vnb;
    }
    // word scores: one back-off walk per live beam whose word part the delimiter may end this frame
    for (int w = tid; w < W; w += 256) {
      if (wlen[w] == 0 || lse2(pb[w], pnb[w]) == NEG || !(y[delim] >= token_min_logp || delim == arg)) continue;
      const int nd = node[w];
      const int word = nd == DEAD ? -1 : L.node_word[nd];
      const int wid = word < 0 ? L.unk_id : word;
      dscore[w] = ((word_lm(L, wh, w, wid)) + (word < 0 ? L.unk_scaled : 0.f)) + L.beta;
      dword[w] = wid;
    }
    __syncthreads();
    // merge: beam w (prefix l' = l + last) absorbs the extension (w0, last) of its parent beam w0
    for (int w = tid; w < W; w += 256) {
      const int l = last[w];
      if (blen[w] == 0 || lse2(pb[w], pnb[w]) == NEG || !(y[l] >= token_min_logp || l == arg)) continue;
      for (int w0 = 0; w0 < W; ++w0) {
        if (w0 != w && hs[w0] == phs[w] && lse2(pb[w0], pnb[w0]) != NEG) {
          const int ke = w0 * C + l;
          cnb[w * C + blank] = lse2(cnb[w * C + blank], cnb[ke]);
          break;
        }
      }
    }
    __syncthreads();
    for (int w = tid; w < W; w += 256) {   // suppress the merged extensions (after every merge read them)
      const int l = last[w];
      if (blen[w] == 0 || lse2(pb[w], pnb[w]) == NEG || !(y[l] >= token_min_logp || l == arg)) continue;
      for (int w0 = 0; w0 < W; ++w0)
        if (w0 != w && hs[w0] == phs[w] && lse2(pb[w0], pnb[w0]) != NEG) {
          cb[w0 * C + l] = NEG;
          cnb[w0 * C + l] = NEG;
          break;
        }
    }
    __syncthreads();
    // rank of every candidate (kept in key[] until the sort keys replace it), best rank. Only
    // candidates that are alive probe the trie: those passed token_min_logp.
    float mx = NEG;
    for (int k = tid; k < np2; k += 256) {
      float rank = NEG;
      if (k < N) {
        const float tot = lse2(cb[k], cnb[k]);
        if (tot != NEG) {
          const int w = k / C, c = k - w * C;
          float a = acc[w];
          int nd = node[w], ln = wlen[w];
          if (c == delim) {
            if (ln > 0) a = a + dscore[w];
            nd = 0;
            ln = 0;
          } else if (c != blank) {
            nd = trie_child(L, nd, c);
            ln = ln + 1;
          }
          rank = (tot + a) + partial_penalty(L, nd, ln);
        }
      }
      key[k] = __float_as_uint(rank);
      mx = fmaxf(mx, rank);
    }
    sh_red[tid] = mx;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
      if (tid < s) sh_red[tid] = fmaxf(sh_red[tid], sh_red[tid + s]);
      __syncthreads();
    }
    if (tid == 0) sh_best = sh_red[0];
    __syncthreads();
    const float thr = sh_best + prune_logp;
    for (int k = tid; k < np2; k += 256) {   // thread tid wrote key[k] above
      const float rank = __uint_as_float((uint32_t)key[k]);
      const bool ok = rank != NEG && rank >= thr;
      // ascending sort of (descending rank, ascending k); dropped candidates last
      key[k] = ok ? ((uint64_t)(~ord(rank)) << 32) | (uint32_t)k : ~0ull;
    }
    __syncthreads();
    for (int size = 2; size <= np2; size <<= 1) {
      for (int stride = size >> 1; stride > 0; stride >>= 1) {
        for (int i = tid; i < np2 / 2; i += 256) {
          const int lo = 2 * i - (i & (stride - 1));
          const int hi = lo + stride;
          const bool asc = (lo & size) == 0;
          const uint64_t a = key[lo], c2 = key[hi];
          if ((a > c2) == asc) {
            key[lo] = c2;
            key[hi] = a;
          }
        }
        __syncthreads();
      }
    }
    // next beams
    for (int w = tid; w < W; w += 256) {
      const uint64_t kk = key[w];
      int32_t rec = -1;
      if (kk == ~0ull) {
        npb[w] = NEG;
        npnb[w] = NEG;
        nhs[w] = 0;
        nphs[w] = 0;
        nlast[w] = -1;
        nlen[w] = 0;
        nnode[w] = 0;
        nwlen[w] = 0;
        for (int j = 0; j < BM_H; ++j) nwh[j][w] = -1;
        nacc[w] = 0.f;
      } else {
        const int k = (int)(uint32_t)kk;
        const int w0 = k / C, c = k - w0 * C;
        npb[w] = cb[k];
        npnb[w] = cnb[k];
        float a = acc[w0];
        int nd = node[w0], ln = wlen[w0];
        const bool word_end = c == delim && ln > 0;
        if (c == blank) {
          nhs[w] = hs[w0];
          nphs[w] = phs[w0];
          nlast[w] = last[w0];
          nlen[w] = blen[w0];
          rec = w0 << 8 | 0xFF;
        } else {
          nhs[w] = hmix(hs[w0], c);
          nphs[w] = hs[w0];
          nlast[w] = c;
          nlen[w] = blen[w0] + 1;
          rec = w0 << 8 | c;
          if (c == delim) {
            if (word_end) a = a + dscore[w0];
            nd = 0;
            ln = 0;
          } else {
            nd = trie_child(L, nd, c);
            ln = ln + 1;
          }
        }
        nnode[w] = nd;
        nwlen[w] = ln;
        nacc[w] = a;
        for (int j = 0; j < BM_H - 1; ++j) nwh[j][w] = wh[word_end ? j + 1 : j][w0];
        nwh[BM_H - 1][w] = word_end ? dword[w0] : wh[BM_H - 1][w0];
      }
      hb[(int64_t)t * W + w] = rec;
    }
    __syncthreads();
    for (int w = tid; w < W; w += 256) {
      pb[w] = npb[w];
      pnb[w] = npnb[w];
      hs[w] = nhs[w];
      phs[w] = nphs[w];
      last[w] = nlast[w];
      blen[w] = nlen[w];
      node[w] = nnode[w];
      wlen[w] = nwlen[w];
      for (int j = 0; j < BM_H; ++j) wh[j][w] = nwh[j][w];
      acc[w] = nacc[w];
    }
    __syncthreads();
  }
  // end of sequence: final rank of every live beam (npb: rank, nacc: LM score, nwh: history after a
  // trailing word)
  for (int w = tid; w < W; w += 256) {
    const float tot = lse2(pb[w], pnb[w]);
    float a = acc[w], rank = NEG;
    if (tot != NEG) {
      const bool word_end = wlen[w] > 0;
      int wid = 0;
      if (word_end) {
        const int nd = node[w];
        const int word = nd == DEAD ? -1 : L.node_word[nd];
        wid = word < 0 ? L.unk_id : word;
        a = a + (((word_lm(L, wh, w, wid)) + (word < 0 ? L.unk_scaled : 0.f)) + L.beta);
      }
      if (L.boundary) {
        for (int j = 0; j < BM_H - 1; ++j) nwh[j][w] = wh[word_end ? j + 1 : j][w];
        nwh[BM_H - 1][w] = word_end ? wid : wh[BM_H - 1][w];
        a = a + word_lm(L, nwh, w, L.eos_id);
      }
      rank = tot + a;
    }
    npb[w] = rank;
    nacc[w] = a;
  }
  __threadfence_block();
  __syncthreads();
  // read back the beam with the best final rank (ties: lower slot; empty prefix when Tb == 0)
  if (tid == 0) {
    int best = 0;
    for (int w = 1; w < W; ++w)
      if (npb[w] > npb[best]) best = w;
    const int n = Tb > 0 ? blen[best] : 0;
    out_len[b] = n;
    out_ctc[b] = Tb > 0 ? lse2(pb[best], pnb[best]) : 0.f;
    out_fused[b] = Tb > 0 ? npb[best] : 0.f;
    int w = best, pos = n;
    for (int t = Tb - 1; t >= 0 && pos > 0; --t) {
      const int32_t rec = hb[(int64_t)t * W + w];
      const int c = rec & 0xFF;
      if (c != 0xFF) out_tok[(int64_t)b * T + (--pos)] = c;
      w = rec >> 8;
    }
    for (int i = n; i < T; ++i) out_tok[(int64_t)b * T + i] = -1;
  }
}

}  // namespace

extern "C" int64_t b2p_ctc_beam_lm_workspace(int64_t B, int64_t T, int64_t beam) { return B * T * beam; }

extern "C" int b2p_ctc_prefix_beam_lm(const float* logits, int64_t B, int64_t T, int64_t C, const int32_t* lens,
                                      int64_t beam, int blank, int delim, float token_min_logp,
                                      float beam_prune_logp, const b2p_ngram_lm* lm, float unk_score_offset,
                                      float unk_score_scaled, int score_boundary, int32_t* workspace,
                                      int32_t* out_tokens, int32_t* out_len, float* out_ctc_logp, float* out_score,
                                      b2p_stream_t stream) {
  B2P_CHECK_ARG(logits && lm && workspace && out_tokens && out_len && out_ctc_logp && out_score,
                "ctc_prefix_beam_lm: NULL pointer");
  B2P_CHECK_ARG(lm->trie_keys && lm->trie_child && lm->node_word && lm->ng_keys && lm->ng_vals,
                "ctc_prefix_beam_lm: NULL pointer in the LM image");
  B2P_CHECK_ARG(lm->order >= 1 && lm->order <= 5, "ctc_prefix_beam_lm: LM order must be in [1, 5]");
  B2P_CHECK_ARG(beam >= 1 && beam <= BM_W, "ctc_prefix_beam_lm: beam width must be in [1, %d]", BM_W);
  B2P_CHECK_ARG(C >= 2 && C <= BM_C && blank >= 0 && blank < C && delim >= 0 && delim < C && delim != blank,
                "ctc_prefix_beam_lm: need 2 <= C <= %d, blank < C, delim < C, delim != blank", BM_C);
  B2P_CHECK_ARG(T >= 0 && beam_prune_logp <= 0.f, "ctc_prefix_beam_lm: T >= 0, beam_prune_logp <= 0");
  const int64_t tc = lm->trie_capacity, gc = lm->ng_capacity;
  B2P_CHECK_ARG(tc >= 2 && tc <= (1ll << 31) && (tc & (tc - 1)) == 0 && gc >= 2 && gc <= (1ll << 31) &&
                    (gc & (gc - 1)) == 0,
                "ctc_prefix_beam_lm: table capacities must be powers of two in [2, 2^31]");
  B2P_CHECK_ARG(lm->unk_id >= 0 && (!score_boundary || (lm->bos_id >= 0 && lm->eos_id >= 0)),
                "ctc_prefix_beam_lm: the LM needs <unk>, and <s> and </s> to score the boundary");
  if (B <= 0) return 0;
  LmImage L;
  L.trie_keys = lm->trie_keys;
  L.trie_child = lm->trie_child;
  L.node_word = lm->node_word;
  L.ng_keys = lm->ng_keys;
  L.ng_vals = reinterpret_cast<const float2*>(lm->ng_vals);
  L.trie_seed = lm->trie_seed;
  L.ng_seed = lm->ng_seed;
  L.trie_mask = (uint32_t)(tc - 1);
  L.ng_mask = (uint32_t)(gc - 1);
  L.order = lm->order;
  L.unk_id = lm->unk_id;
  L.bos_id = lm->bos_id;
  L.eos_id = lm->eos_id;
  L.beta = lm->beta;
  L.unk_scaled = unk_score_scaled;
  L.unk_offset = unk_score_offset;
  L.boundary = score_boundary != 0;
  hipLaunchKernelGGL(ctc_beam_lm_k, dim3((unsigned)B), dim3(256), 0, (hipStream_t)stream, logits, (int)T, (int)C,
                     lens, (int)beam, blank, delim, token_min_logp, beam_prune_logp, L, workspace, out_tokens, out_len,
                     out_ctc_logp, out_score);
  B2P_CHECK_LAUNCH();
  return 0;
}
