// Multi-CU persistent GRU recurrence (nn.GRU semantics, gate order r, z, n) for hidden sizes too
// large for one CU (the Conformer experiment's brain encoder: H = 512 x 3 layers, reference
// src/model/brain_feature_extractor.py:39-47, 56-68; README encoder H512x3), bf16 precision mode.
//
// One launch runs the whole time loop. A recurrence (direction d, 16 batch rows) is spread over
// P = H/64 workgroups ("members"), one per CU: member m owns hidden units [64m, 64m+64) and keeps
// their W_hh rows (r, z, n: 192 x H; fp16 in the forward, bf16 in the backward) in registers as MFMA
// A-fragments for the whole launch, so W_hh is read from HBM once per launch instead of once per
// step. Per step the members exchange the new state through L2 as tagged 8-byte granules ({tag =
// step+1, two fp16 h values / three bf16 dgh values}: written by one sc1
// store, polled by sc1 loads until every tag matches; MI355X_MICROARCH.md 'Workgroup dispatch, XCD
// placement & inter-workgroup visibility', cdna_hip_programming.md Guideline 16 R2) — no fences,
// no flags, no grid barrier. The exchange slots are zeroed by a memset before every launch (so tags
// of a previous launch or graph replay never match) and double-buffered by step parity (a member
// can be at most one step ahead of any other). Workgroups of one recurrence take block ids with
// equal blockIdx % 8 (one XCD under the observed round-robin placement: speed only).
// H = 1024 (the reference sweeps' largest encoder) is the same template at P = 16 with three differences,
// all under `H == 1024`: the W_hh fragments (384 registers per lane) sit in AGPRs, VGPRs and LDS and the
// MFMAs read the AGPR ones in place (see "MFMAs that read W_hh straight from AGPRs"); the exchange is swept
// in parts and the backward keeps one dgh image; and a batch of more than LAUNCH_BUDGET workgroups runs
// as successive launches over disjoint batch groups (launch_mc).
//
//   forward : gates^T (3 x 64 x 16) = W_hh[rows of m] (192 x H) . h_{t-1}^T (H x 16), fp32 acc
//   backward: dh_rec^T (64 x 16)    = W_hh[:, units of m]^T (64 x 3H) . dgh_{t+1}^T (3H x 16)
// Inputs / outputs use the standard layouts of the per-step kernels (csrc/gru.hip), so these are
// drop-in for b2p_gru_fwd / b2p_gru_bwd: gi, dgi, dgh [B][T][ndir*3H], out [B][T][ndir*H],
// saved [B][T][ndir][4][H] = (r, z, n, W_hn h + b_hn), h0 / dh0 [ndir][B][H].
#include "common.h"
#include "gru_dev.h"   // BG, sigm, tanh_fast, pack8_strided
#include "gru_xch.h"   // granules, sweep, place, same_xcd, workspace and argument checks: shared with csrc/gru32.hip
#include "../../include/b2p_hip.h"

namespace {
constexpr int UPM = 64;       // hidden units per member
constexpr int NTH = XCH_NTH;  // 4 waves x 16 units
constexpr int MAX_GROUPS = 32;      // (direction, 16-row batch group) recurrences per launch
constexpr int64_t HDR_BYTES = 16 + (int64_t)MAX_GROUPS * IDS_PER_GROUP * 8;   // fail word + ids
constexpr int LAUNCH_BUDGET = 128;  // workgroups per launch at H = 1024 (csrc/gru32.hip: half the chip's CUs)

// H = 1024: a wave's W_hh fragments alone are 384 of the 512 registers a lane has (VGPR + AGPR at one wave
// per SIMD), so what else is live is cut: the exchange is swept SW1024 granules per lane at a time instead
// of all NGR at once (the sweep keeps every granule it polls in registers), and the backward keeps ONE dgh
// image (two would be 197,120 B of LDS) behind one more barrier per step.
constexpr int SW1024 = 16;
template <int H>
constexpr int sweep_width(int ngr) { return H == 1024 ? SW1024 : ngr; }
template <int H>
constexpr int bwd_images() { return H == 1024 ? 1 : 2; }
// (sweep_parts, csrc/gru_xch.h: SW granules per sweep call)

__device__ __forceinline__ unsigned pack2(float a, float b) {
  return (unsigned)b2p_bf16_bits(a) | ((unsigned)b2p_bf16_bits(b) << 16);
}
__device__ __forceinline__ unsigned pack2h(float a, float b) {
  return (unsigned)b2p_f16_bits(a) | ((unsigned)b2p_f16_bits(b) << 16);
}
__device__ __forceinline__ float4 f4(const f32x4& a) { return make_float4(a[0], a[1], a[2], a[3]); }

// ---- H = 1024: MFMAs that read W_hh straight from AGPRs.
// A wave's W_hh fragments are 384 registers, and a lane has 256 VGPRs + 256 AGPRs. The compiler allocates an
// MFMA builtin's A operand in VGPRs and uses AGPRs only as a parking place (one v_accvgpr_read per register
// and MFMA: 232 per step in grumc_fwd<512>), which at this size ends in scratch. So the first KA_* k-steps'
// fragments are handed to the MFMA with an "a" constraint (the instruction reads A / B from either file) and
// stay in AGPRs for the whole launch; the rest are "v". Nothing inside an asm string is padded by the
// compiler: "s_nop 1" covers a just-written operand (the accumulators' initial values, a v_accvgpr_write in
// the prologue), an accumulator goes from one statement to the next only as the whole C of the same
// chain (no wait), and the last k-step's statement ends with the wait of its results' way to any other reader
// (8-pass XDL: 12 states; "s_nop 15" inside the string, so that no compiler copy can come before it).
typedef __attribute__((ext_vector_type(4))) unsigned u32x4;
__device__ __forceinline__ u32x4 as_u4(const bf16x8& a) { return __builtin_bit_cast(u32x4, a); }
constexpr int KA_FWD = 21;   // of 32 k-steps x 3 gates: 63 fragments = 252 AGPRs
constexpr int KA_BWD = 64;   // of 96 k-steps: 256 AGPRs
// The last k-steps' fragments stay in LDS behind the state image ([fragment][thread] 16 B: one conflict-free
// ds_read_b128 per fragment and step), which leaves the VGPRs the rest of the step needs.
constexpr int KL_FWD = 29;   // k-steps 29..31 x 3 gates: 9 fragments, 36 KB
constexpr int KL_BWD = 82;   // k-steps 82..95: 14 fragments, 56 KB
constexpr size_t FRAG_BYTES = (size_t)XCH_NTH * 16;
#define B2P_MFMA3(NAME, OP, CA, END)                                                                             \
  __device__ __forceinline__ void NAME(f32x4& c0, f32x4& c1, f32x4& c2, u32x4 a0, u32x4 a1, u32x4 a2, u32x4 b) { \
    asm("s_nop 1\n\t" OP " %0, %3, %6, %0\n\t" OP " %1, %4, %6, %1\n\t" OP " %2, %5, %6, %2" END                  \
        : "+v"(c0), "+v"(c1), "+v"(c2)                                                                             \
        : CA(a0), CA(a1), CA(a2), "v"(b));                                                                         \
  }
#define B2P_MFMA2(NAME, OP, CA, END)                                                                   \
  __device__ __forceinline__ void NAME(f32x4& c0, f32x4& c1, u32x4 a0, u32x4 a1, u32x4 b0, u32x4 b1) { \
    asm("s_nop 1\n\t" OP " %0, %2, %4, %0\n\t" OP " %1, %3, %5, %1" END                                \
        : "+v"(c0), "+v"(c1)                                                                           \
        : CA(a0), CA(a1), "v"(b0), "v"(b1));                                                           \
  }
B2P_MFMA3(mfma3_f16_a, "v_mfma_f32_16x16x32_f16", "a", "")
B2P_MFMA3(mfma3_f16_v, "v_mfma_f32_16x16x32_f16", "v", "")
B2P_MFMA3(mfma3_f16_v_last, "v_mfma_f32_16x16x32_f16", "v", "\n\ts_nop 15")
B2P_MFMA2(mfma2_bf16_a, "v_mfma_f32_16x16x32_bf16", "a", "")
B2P_MFMA2(mfma2_bf16_v, "v_mfma_f32_16x16x32_bf16", "v", "")
B2P_MFMA2(mfma2_bf16_v_last, "v_mfma_f32_16x16x32_bf16", "v", "\n\ts_nop 15")
#undef B2P_MFMA3
#undef B2P_MFMA2
// prologue: a fragment is converted and put in its file before the next one's fp32 loads are issued (left
// alone, all 768 fp32 registers' worth of loads comes first)
__device__ __forceinline__ void pin_frag(bf16x8& f, bool agpr) {
  u32x4 t = as_u4(f);
  if (agpr) asm volatile("" : "+a"(t));
  else asm volatile("" : "+v"(t));
  f = __builtin_bit_cast(bf16x8, t);
  __builtin_amdgcn_sched_barrier(0);
}

// ------------------------------------------------------------------------------------------ forward
// exchange slots: [group][2][P * 512] granules (h_s of member m, batch b, unit pair p at
// m*512 + b*32 + p)
template <int H>
__global__ void __launch_bounds__(NTH, 1) grumc_fwd(const float* __restrict__ gi, const float* __restrict__ whh,
                                                    const float* __restrict__ bhh, const float* __restrict__ h0,
                                                    float* __restrict__ out, float* __restrict__ saved,
                                                    unsigned long long* xch, unsigned long long* ids, int* fail, int B,
                                                    int T, int ndir, int nbg, int withhold, int nbg_all, int bg0) {
  constexpr int P = H / UPM;
  constexpr int KS = H / 32;
  constexpr int HPW = H / 2 + 4;              // u32 words per batch row of the h image (16-B stagger)
  constexpr int NGR = P * 512 / NTH;          // granules swept per lane
  constexpr int SW = sweep_width<H>(NGR);     // of them per sweep call
  constexpr int G3 = 3 * H;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  unsigned* hw = reinterpret_cast<unsigned*>(smem);   // [2][BG][HPW] u32 (fp16 pairs)
  u32x4* wl = reinterpret_cast<u32x4*>(smem + (size_t)2 * BG * HPW * 4);   // H = 1024: W_hh fragments of k-steps >= KL_FWD

  int d, bgl, m;
  if (!place(P, ndir * nbg, d, bgl, m, nbg)) return;
  // chunked launches (H = 1024 only): bg0 = first batch group of this launch, nbg_all = the layer's
  const int bg = H == 1024 ? bg0 + bgl : bgl;
  const int tid = threadIdx.x, w = tid >> 6, l = tid & 63, lr = l & 15, lq = l >> 4;
  const int b = bg * BG + lr;
  const bool bok = b < B;
  const int u0 = m * UPM + w * 16;             // first unit of this wave's block
  const int j0 = u0 + 4 * lq;                  // this lane's 4 output units
  const float* W = whh + (int64_t)d * G3 * H;
  const int gg = d * (H == 1024 ? nbg_all : nbg) + bg;
  unsigned long long* xg = xch + (int64_t)gg * 2 * P * 512;
  bool dead = false;
  const bool local = same_xcd(ids + gg * IDS_PER_GROUP, P, m, fail, dead);

  bf16x8 wf[3][KS];
#pragma unroll
  for (int g = 0; g < 3; ++g)
#pragma unroll
    for (int s = 0; s < KS; ++s) {
      wf[g][s] = b2p_pack8_f16(W + (int64_t)(g * H + u0 + lr) * H + 32 * s + 8 * lq);
      if constexpr (H == 1024) {
        if (s >= KL_FWD) wl[((s - KL_FWD) * 3 + g) * NTH + tid] = as_u4(wf[g][s]);
        else pin_frag(wf[g][s], s < KA_FWD);
      }
    }
  float4 bh[3];
#pragma unroll
  for (int g = 0; g < 3; ++g)
    bh[g] = bhh ? *reinterpret_cast<const float4*>(bhh + (int64_t)d * G3 + g * H + j0) : make_float4(0.f, 0.f, 0.f, 0.f);

  // h_{-1}: h0 (or zeros) straight into image 0, and this lane's own 4 values in registers
  float hp[4] = {0.f, 0.f, 0.f, 0.f};
  for (int i = tid; i < BG * (H / 2); i += NTH) {
    const int r = i / (H / 2), c = i % (H / 2);
    const int bb = bg * BG + r;
    float a = 0.f, c2 = 0.f;
    if (h0 && bb < B) {
      a = h0[((int64_t)d * B + bb) * H + 2 * c];
      c2 = h0[((int64_t)d * B + bb) * H + 2 * c + 1];
    }
    hw[r * HPW + c] = pack2h(a, c2);
  }
  if (h0 && bok) {
    const float4 v = *reinterpret_cast<const float4*>(h0 + ((int64_t)d * B + b) * H + j0);
    hp[0] = v.x; hp[1] = v.y; hp[2] = v.z; hp[3] = v.w;
  }
  __syncthreads();

  const int64_t gstride = (int64_t)ndir * G3, ostride = (int64_t)ndir * H;
  // vmcnt counts loads and stores together, in issue order, so the granule stores go out first in a
  // step; the outputs and the next step's input loads follow and complete while the other members
  // are still on their way to the next exchange.
  auto load_gi = [&](int s, float4 (&g)[3]) {
    const int t = d == 0 ? s : T - 1 - s;
    const float* gp = gi + ((int64_t)b * T + t) * gstride + d * G3 + j0;
    if (bok)
#pragma unroll
      for (int q = 0; q < 3; ++q) g[q] = *reinterpret_cast<const float4*>(gp + q * H);
  };
  float4 gc[3];   // this step's input projection (the next step's is loaded into it once consumed)
#pragma unroll
  for (int q = 0; q < 3; ++q) gc[q] = make_float4(0.f, 0.f, 0.f, 0.f);
  load_gi(0, gc);
  float st_h[4], st_r[4], st_z[4], st_n[4], st_g[4];   // this step's outputs
  auto store_out = [&](int s) {
    if (!bok) return;
    const int t = d == 0 ? s : T - 1 - s;
    *reinterpret_cast<float4*>(out + ((int64_t)b * T + t) * ostride + d * H + j0) =
        make_float4(st_h[0], st_h[1], st_h[2], st_h[3]);
    float* sv = saved + (((int64_t)b * T + t) * ndir + d) * 4 * H + j0;
    *reinterpret_cast<float4*>(sv) = make_float4(st_r[0], st_r[1], st_r[2], st_r[3]);
    *reinterpret_cast<float4*>(sv + H) = make_float4(st_z[0], st_z[1], st_z[2], st_z[3]);
    *reinterpret_cast<float4*>(sv + 2 * H) = make_float4(st_n[0], st_n[1], st_n[2], st_n[3]);
    *reinterpret_cast<float4*>(sv + 3 * H) = make_float4(st_g[0], st_g[1], st_g[2], st_g[3]);
  };
  for (int s = 0; s < T; ++s) {
    float4 (&g)[3] = gc;
    if (s > 0) {   // h_{s-1} of every member: tags s, slot (s-1) & 1 -> image s & 1
      unsigned* img = hw + (s & 1) * BG * HPW;
      const unsigned tag = (unsigned)s;
      sweep_parts<NGR, SW>(xg + ((s - 1) & 1) * P * 512, [tag](unsigned long long x) { return (unsigned)(x >> 32) == tag; },
                 [&](int q, unsigned long long x) { img[((q >> 5) & 15) * HPW + (q >> 9) * 32 + (q & 31)] = (unsigned)x; },
                 fail, dead);
      __syncthreads();
    }
    // gate pre-activations: acc = gi + b_hh (r, z) / b_hn (n) + W . h
    f32x4 acc[3];
    acc[0] = f32x4{g[0].x + bh[0].x, g[0].y + bh[0].y, g[0].z + bh[0].z, g[0].w + bh[0].w};
    acc[1] = f32x4{g[1].x + bh[1].x, g[1].y + bh[1].y, g[1].z + bh[1].z, g[1].w + bh[1].w};
    acc[2] = f32x4{bh[2].x, bh[2].y, bh[2].z, bh[2].w};
    const unsigned* hrow = hw + (s & 1) * BG * HPW + lr * HPW + 4 * lq;
    if constexpr (H == 1024) {
      u32x4 nb = *reinterpret_cast<const u32x4*>(hrow);   // the h fragment is read one k-step ahead of its MFMAs
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) {
        const u32x4 bf = nb;
        if (ks + 1 < KS) nb = *reinterpret_cast<const u32x4*>(hrow + 16 * (ks + 1));
        if (ks < KA_FWD) mfma3_f16_a(acc[0], acc[1], acc[2], as_u4(wf[0][ks]), as_u4(wf[1][ks]), as_u4(wf[2][ks]), bf);
        else if (ks < KL_FWD) mfma3_f16_v(acc[0], acc[1], acc[2], as_u4(wf[0][ks]), as_u4(wf[1][ks]), as_u4(wf[2][ks]), bf);
        else {
          const u32x4* wp = wl + (ks - KL_FWD) * 3 * NTH + tid;
          if (ks < KS - 1) mfma3_f16_v(acc[0], acc[1], acc[2], wp[0], wp[NTH], wp[2 * NTH], bf);
          else mfma3_f16_v_last(acc[0], acc[1], acc[2], wp[0], wp[NTH], wp[2 * NTH], bf);
        }
      }
    } else {
#pragma unroll
      for (int ks = 0; ks < KS; ++ks) {
        const bf16x8 bf = *reinterpret_cast<const bf16x8*>(hrow + 16 * ks);
#pragma unroll
        for (int q = 0; q < 3; ++q) acc[q] = b2p_mfma_f16(wf[q][ks], bf, acc[q]);
      }
    }
    const float gnv[4] = {g[2].x, g[2].y, g[2].z, g[2].w};
    float hh[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const float rr = sigm(acc[0][i]);
      const float zz = sigm(acc[1][i]);
      const float nn = tanh_fast(gnv[i] + rr * acc[2][i]);
      hh[i] = bok ? (1.f - zz) * nn + zz * hp[i] : 0.f;
      hp[i] = hh[i];
      st_h[i] = hh[i];
      st_r[i] = rr;
      st_z[i] = zz;
      st_n[i] = nn;
      st_g[i] = acc[2][i];
    }
    // publish h_s (fp16 pairs) FIRST: the other members wait on it, and a later store or load issued
    // before it would delay it; then this step's outputs and the next step's input projection
    if (s + 1 < T && m != withhold) {   // withhold: test knob (b2p_gru_mc_debug_withhold), -1 = off
      unsigned long long* dst = xg + (s & 1) * P * 512 + m * 512 + lr * 32 + w * 8 + lq * 2;
      put_granule(dst, (unsigned)(s + 1), pack2h(hh[0], hh[1]), local);
      put_granule(dst + 1, (unsigned)(s + 1), pack2h(hh[2], hh[3]), local);
    }
    store_out(s);
    if (s + 1 < T) load_gi(s + 1, gc);
  }
}

// ----------------------------------------------------------------------------------------- backward
// Processing steps run backwards (s = T-1 .. 0, t = t(s)). For own units j:
//   dh_s = dout[t] + [s < T-1] (z_{s+1} dh_{s+1} + (W^T dgh_{s+1})_j)
//   dn = dh (1-z); dz = dh (h_{s-1} - n); dan = dn (1 - n^2); dar = dan ghn r (1-r); daz = dz z (1-z)
//   dgi = (dar, daz, dan), dgh = (dar, daz, dan r)
// The reduction runs over all 3H gate rows in the interleaved order k = 3*unit + gate, so one unit's
// three dgh values travel in ONE granule {bf16 r, bf16 z | bf16 n, 16-bit tag} and land as three
// consecutive bf16 of the LDS image; W^T's A-fragments are gathered in the same order.
// exchange slots: [group][2][P * 1024] granules (member m, batch b, unit u of m at m*1024 + b*64 + u)
__device__ __forceinline__ unsigned long long dgh_granule(float r, float z, float n, unsigned tag) {
  return (unsigned long long)pack2(r, z) | ((unsigned long long)(b2p_bf16_bits(n) | (tag << 16)) << 32);
}

template <int H>
__global__ void __launch_bounds__(NTH, 1) grumc_bwd(const float* __restrict__ dout, const float* __restrict__ whh,
                                                    const float* __restrict__ out, const float* __restrict__ saved,
                                                    const float* __restrict__ h0, float* __restrict__ dgi,
                                                    float* __restrict__ dgh, float* __restrict__ dh0,
                                                    unsigned long long* xch, unsigned long long* ids, int* fail, int B,
                                                    int T, int ndir, int nbg, int withhold, int nbg_all, int bg0) {
  constexpr int P = H / UPM;
  constexpr int G3 = 3 * H;
  constexpr int KS = G3 / 32;                  // k-steps over all gate rows
  constexpr int GPH = G3 + 8;                  // bf16 per batch row of the dgh image (16-B stagger)
  constexpr int NGR = P * 1024 / NTH;
  constexpr int SW = sweep_width<H>(NGR);
  constexpr int NIMG = bwd_images<H>();        // 2: by step parity; 1: one more barrier per step instead
  extern __shared__ __attribute__((aligned(16))) char smem[];
  uint16_t* gimg = reinterpret_cast<uint16_t*>(smem);   // [NIMG][BG][GPH] bf16, k = 3*unit + gate
  u32x4* wl = reinterpret_cast<u32x4*>(smem + (size_t)NIMG * BG * GPH * 2);   // H = 1024: W^T fragments of k-steps >= KL_BWD

  int d, bgl, m;
  if (!place(P, ndir * nbg, d, bgl, m, nbg)) return;
  // chunked launches (H = 1024 only): bg0 = first batch group of this launch, nbg_all = the layer's
  const int bg = H == 1024 ? bg0 + bgl : bgl;
  const int tid = threadIdx.x, w = tid >> 6, l = tid & 63, lr = l & 15, lq = l >> 4;
  const int b = bg * BG + lr;
  const bool bok = b < B;
  const int u0 = m * UPM + w * 16;
  const int j0 = u0 + 4 * lq;
  const float* W = whh + (int64_t)d * G3 * H;
  const int gg = d * (H == 1024 ? nbg_all : nbg) + bg;
  unsigned long long* xg = xch + (int64_t)gg * 2 * P * 1024;
  bool dead = false;
  const bool local = same_xcd(ids + gg * IDS_PER_GROUP, P, m, fail, dead);

  // A = W^T in the interleaved k order: lane holds W[gate(k)*H + unit(k)][u0 + lr], k = 32s + 8lq + i
  bf16x8 wt[KS];
#pragma unroll
  for (int s = 0; s < KS; ++s) {
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int k = 32 * s + 8 * lq + i;
      wt[s][i] = (__bf16)W[(int64_t)((k % 3) * H + k / 3) * H + u0 + lr];
    }
    if constexpr (H == 1024) {
      if (s >= KL_BWD) wl[(s - KL_BWD) * NTH + tid] = as_u4(wt[s]);
      else pin_frag(wt[s], s < KA_BWD);
    }
  }

  float dhn[4] = {0.f, 0.f, 0.f, 0.f}, zn[4] = {0.f, 0.f, 0.f, 0.f};
  const int64_t gstride = (int64_t)ndir * G3, ostride = (int64_t)ndir * H;
  // as in the forward: granules first, then this step's outputs, then the next step's inputs
  auto load_in = [&](int s, float4 (&v)[6]) __attribute__((always_inline)) {   // dout, r, z, n, ghn, h_{s-1}
    if (!bok) return;
    const int t = d == 0 ? s : T - 1 - s;
    const int tp = d == 0 ? t - 1 : t + 1;
    v[0] = *reinterpret_cast<const float4*>(dout + ((int64_t)b * T + t) * ostride + d * H + j0);
    const float* sv = saved + (((int64_t)b * T + t) * ndir + d) * 4 * H + j0;
#pragma unroll
    for (int q = 0; q < 4; ++q) v[1 + q] = *reinterpret_cast<const float4*>(sv + q * H);
    if (s > 0) v[5] = *reinterpret_cast<const float4*>(out + ((int64_t)b * T + tp) * ostride + d * H + j0);
    else if (h0) v[5] = *reinterpret_cast<const float4*>(h0 + ((int64_t)d * B + b) * H + j0);
    else v[5] = make_float4(0.f, 0.f, 0.f, 0.f);   // h_{-1} = 0 (the buffer still holds step 1's h_0)
  };
  float4 ic[6];
#pragma unroll
  for (int q = 0; q < 6; ++q) ic[q] = make_float4(0.f, 0.f, 0.f, 0.f);
  load_in(T - 1, ic);
  float st_ar[4], st_az[4], st_an[4], st_r[4];   // this step's outputs
  auto store_out = [&](int s) __attribute__((always_inline)) {
    if (!bok) return;
    const int t = d == 0 ? s : T - 1 - s;
    float* gp = dgi + ((int64_t)b * T + t) * gstride + d * G3 + j0;
    float* hq = dgh + ((int64_t)b * T + t) * gstride + d * G3 + j0;
    const float4 a4 = make_float4(st_ar[0], st_ar[1], st_ar[2], st_ar[3]);
    const float4 z4 = make_float4(st_az[0], st_az[1], st_az[2], st_az[3]);
    *reinterpret_cast<float4*>(gp) = a4;
    *reinterpret_cast<float4*>(gp + H) = z4;
    *reinterpret_cast<float4*>(gp + 2 * H) = make_float4(st_an[0], st_an[1], st_an[2], st_an[3]);
    *reinterpret_cast<float4*>(hq) = a4;
    *reinterpret_cast<float4*>(hq + H) = z4;
    *reinterpret_cast<float4*>(hq + 2 * H) = make_float4(st_an[0] * st_r[0], st_an[1] * st_r[1], st_an[2] * st_r[2],
                                                         st_an[3] * st_r[3]);
  };
  // W^T . dgh_{s+1} from the exchange (tag s+2, slot (s+1) & 1 -> image (s+1) & 1)
  auto recur = [&](int s) __attribute__((always_inline)) {
    uint16_t* img = gimg + ((s + 1) & (NIMG - 1)) * BG * GPH;
    const unsigned tag = (unsigned)(s + 2);
    // one image: no wave may refill it before every wave has read the previous step's fragments
    if constexpr (NIMG == 1) __syncthreads();
    sweep_parts<NGR, SW>(xg + ((s + 1) & 1) * P * 1024, [tag](unsigned long long x) { return (unsigned)(x >> 48) == tag; },
               [&](int q, unsigned long long x) {
                 const int mm = q >> 10, bb = (q >> 6) & 15, u = q & 63;
                 const int k = 3 * (mm * UPM + u);
                 uint16_t* p = img + bb * GPH + k;
                 const unsigned lo = (unsigned)x, n = (unsigned)(x >> 32) & 0xFFFFu;
                 if (k & 1) {          // r at an odd position: r, then (z, n) as one aligned word
                   p[0] = (uint16_t)lo;
                   *reinterpret_cast<unsigned*>(p + 1) = (lo >> 16) | (n << 16);
                 } else {              // (r, z) as one aligned word, then n
                   *reinterpret_cast<unsigned*>(p) = lo;
                   p[2] = (uint16_t)n;
                 }
               }, fail, dead);
    __syncthreads();
    // two independent accumulation chains (even / odd k-steps): the MFMA pipe never waits on the
    // previous MFMA's result
    f32x4 a0 = f32x4{0.f, 0.f, 0.f, 0.f}, a1 = a0;
    const uint16_t* grow = img + lr * GPH + 8 * lq;
    if constexpr (H == 1024) {
      u32x4 n0 = *reinterpret_cast<const u32x4*>(grow);   // the dgh fragments are read one pair ahead of their MFMAs
      u32x4 n1 = *reinterpret_cast<const u32x4*>(grow + 32);
#pragma unroll
      for (int ks = 0; ks < KS; ks += 2) {
        const u32x4 b0 = n0, b1 = n1;
        if (ks + 2 < KS) {
          n0 = *reinterpret_cast<const u32x4*>(grow + 32 * (ks + 2));
          n1 = *reinterpret_cast<const u32x4*>(grow + 32 * (ks + 3));
        }
        if (ks < KA_BWD) mfma2_bf16_a(a0, a1, as_u4(wt[ks]), as_u4(wt[ks + 1]), b0, b1);
        else if (ks < KL_BWD) mfma2_bf16_v(a0, a1, as_u4(wt[ks]), as_u4(wt[ks + 1]), b0, b1);
        else {
          const u32x4* wp = wl + (ks - KL_BWD) * NTH + tid;
          if (ks < KS - 2) mfma2_bf16_v(a0, a1, wp[0], wp[NTH], b0, b1);
          else mfma2_bf16_v_last(a0, a1, wp[0], wp[NTH], b0, b1);
        }
      }
    } else {
#pragma unroll
      for (int ks = 0; ks < KS; ks += 2) {
        const bf16x8 b0 = *reinterpret_cast<const bf16x8*>(grow + 32 * ks);
        const bf16x8 b1 = *reinterpret_cast<const bf16x8*>(grow + 32 * (ks + 1));
        a0 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wt[ks], b0, a0, 0, 0, 0);
        a1 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wt[ks + 1], b1, a1, 0, 0, 0);
      }
    }
    return f32x4{a0[0] + a1[0], a0[1] + a1[1], a0[2] + a1[2], a0[3] + a1[3]};
  };
  // one input buffer: step s-1's inputs are loaded once step s has consumed them (behind the publish,
  // so they overlap the other members' arrival)
  for (int s = T - 1; s >= 0; --s) {
    f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
    if (s < T - 1) acc = recur(s);
    const float dv[4] = {ic[0].x, ic[0].y, ic[0].z, ic[0].w}, r4[4] = {ic[1].x, ic[1].y, ic[1].z, ic[1].w};
    const float z4[4] = {ic[2].x, ic[2].y, ic[2].z, ic[2].w}, n4[4] = {ic[3].x, ic[3].y, ic[3].z, ic[3].w};
    const float g4[4] = {ic[4].x, ic[4].y, ic[4].z, ic[4].w}, h4[4] = {ic[5].x, ic[5].y, ic[5].z, ic[5].w};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const float dh = dv[i] + (s < T - 1 ? acc[i] + zn[i] * dhn[i] : 0.f);
      const float dn = dh * (1.f - z4[i]);
      const float dz = dh * (h4[i] - n4[i]);
      const float dan = dn * (1.f - n4[i] * n4[i]);
      st_ar[i] = bok ? dan * g4[i] * r4[i] * (1.f - r4[i]) : 0.f;
      st_az[i] = bok ? dz * z4[i] * (1.f - z4[i]) : 0.f;
      st_an[i] = bok ? dan : 0.f;
      st_r[i] = r4[i];
      dhn[i] = bok ? dh : 0.f;
      zn[i] = z4[i];
    }
    if ((s > 0 || dh0) && m != withhold) {   // the step before (or dh0) needs this step's dgh
      unsigned long long* dst = xg + (s & 1) * P * 1024 + m * 1024 + lr * 64 + w * 16 + lq * 4;
      const unsigned tag = (unsigned)(s + 1);
#pragma unroll
      for (int i = 0; i < 4; ++i)
        store_granule(dst + i, dgh_granule(st_ar[i], st_az[i], st_an[i] * st_r[i], tag), local);
    }
    store_out(s);
    if (s > 0) load_in(s - 1, ic);
  }
  if (dh0) {   // dh0 = W^T dgh_0 + z_0 dh_0
    const f32x4 acc = recur(-1);
    if (bok)
      *reinterpret_cast<float4*>(dh0 + ((int64_t)d * B + b) * H + j0) =
          make_float4(acc[0] + zn[0] * dhn[0], acc[1] + zn[1] * dhn[1], acc[2] + zn[2] * dhn[2], acc[3] + zn[3] * dhn[3]);
  }
}

template <int H>
constexpr size_t fwd_lds() { return (size_t)2 * BG * (H / 2 + 4) * 4 + (H == 1024 ? (32 - KL_FWD) * 3 * FRAG_BYTES : 0); }
template <int H>
constexpr size_t bwd_lds() {
  return (size_t)bwd_images<H>() * BG * (3 * H + 8) * 2 + (H == 1024 ? (96 - KL_BWD) * FRAG_BYTES : 0);
}
static_assert(fwd_lds<1024>() <= 163840 && bwd_lds<1024>() <= 163840, "a CU has 160 KB of LDS");

// test knob (b2p_gru_mc_debug_withhold): this member skips its granule stores, so the others time out
int g_withhold = -1;

// Every member of a launch must be resident. H <= 512: one launch (mc_prepare bounds the recurrences by the
// chip's 256 CUs). H = 1024 (P = 16): as csrc/gru32.hip, at most LAUNCH_BUDGET workgroups per launch, so a
// larger batch runs as successive launches on the stream over disjoint 16-row batch groups, both
// directions of a batch group in the same launch, each recurrence on its own part of the workspace.
inline int groups_per_launch(int64_t H, int ndir, int nbg_all) {
  if (H != 1024) return nbg_all;
  const int nb = LAUNCH_BUDGET / (int)(H / UPM) / ndir;
  return nb < 1 ? 1 : nb;
}

// the launch(es) of `kernel` (its tensors in args, then the carved workspace and the shape)
template <auto kernel, int H, size_t LDS, typename... A>
int launch_mc(const XchWs& w, int B, int T, int ndir, hipStream_t st, A... args) {
  static bool attr = false;
  if (!attr) {
    B2P_CHECK_HIP(hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)LDS));
    attr = true;
  }
  const int nbg_all = (B + BG - 1) / BG, step = groups_per_launch(H, ndir, nbg_all);
  for (int bg0 = 0; bg0 < nbg_all; bg0 += step) {
    const int nbg = nbg_all - bg0 < step ? nbg_all - bg0 : step;
    hipLaunchKernelGGL(kernel, dim3(grid_blocks(H / UPM, ndir * nbg)), dim3(NTH), LDS, st, args..., w.xch, w.ids,
                       w.fail, B, T, ndir, nbg, g_withhold, nbg_all, bg0);
    B2P_CHECK_LAUNCH();
  }
  return 0;
}
template <int H, typename... A>
int launch_fwd(A... a) { return launch_mc<grumc_fwd<H>, H, fwd_lds<H>()>(a...); }
template <int H, typename... A>
int launch_bwd(A... a) { return launch_mc<grumc_bwd<H>, H, bwd_lds<H>()>(a...); }

bool mc_supported(int64_t H) { return H == 256 || H == 384 || H == 512 || H == 1024; }
// fail word + ids: MAX_GROUPS recurrences' for the single-launch sizes, every recurrence's at H = 1024
int64_t hdr_bytes(int64_t B, int64_t H, int ndir) {
  return H == 1024 ? 16 + (int64_t)ndir * ((B + BG - 1) / BG) * IDS_PER_GROUP * 8 : HDR_BYTES;
}

__global__ void mc_status_k(const int* __restrict__ fail, int32_t* status, int32_t code) {
  if (threadIdx.x == 0 && fail[0] != 0) atomicCAS(status, 0, code);
}
}  // namespace

extern "C" int b2p_gru_mc_supported(int64_t H) { return mc_supported(H) ? 1 : 0; }

extern "C" int b2p_gru_mc_status(const void* workspace, int32_t* status, int32_t code, b2p_stream_t stream) {
  B2P_CHECK_ARG(workspace && status, "gru_mc_status: NULL pointer");
  B2P_CHECK_ARG(code != 0, "gru_mc_status: code must be nonzero");
  hipLaunchKernelGGL(mc_status_k, dim3(1), dim3(64), 0, (hipStream_t)stream, (const int*)workspace, status, code);
  B2P_CHECK_LAUNCH();
  return 0;
}

extern "C" int b2p_gru_mc_debug_withhold(int member) {
  B2P_CHECK_ARG(member >= -1 && member < 16, "gru_mc_debug_withhold: member must be -1 (off) or 0..15");
  g_withhold = member;
  return 0;
}

// [fail word block 16 B][ids][exchange slots: 2 x P * 1024 granules per recurrence]
extern "C" int64_t b2p_gru_mc_workspace(int64_t B, int64_t H, int ndir) {
  if (!mc_supported(H)) return 0;
  if (B < 0) B = 0;
  const int64_t nbg = (B + BG - 1) / BG, P = H / UPM;
  return hdr_bytes(B, H, ndir) + (int64_t)ndir * nbg * 2 * P * 1024 * 8;   // sized for the backward (2x the forward)
}

// The checks of both entry points (max_T: the backward granule carries a 16-bit step tag, dgh_granule, and tags
// 1..T must stay distinct), then every polled word (tags) and the fail flag zeroed (the backward's size in both
// passes) and the workspace carved. 0 go on, 1 / 2 error set, -1 nothing to do.
static int mc_prepare(const char* who, bool pointers, void* ws, int64_t B, int64_t T, int64_t max_T, int64_t H,
                      int ndir, hipStream_t st, XchWs* w) {
  if (int r = xch_check_args(who, pointers, mc_supported(H), H, "256, 384, 512 or 1024", ndir, ws, B, T)) return r;
  B2P_CHECK_ARG(H != 1024 || (B < (1ll << 24) && T < (1ll << 30)), "%s: B or T out of range", who);   // no CU bound on B there
  const int nbg = (int)((B + BG - 1) / BG);
  B2P_CHECK_ARG(H == 1024 || (grid_blocks((int)(H / UPM), ndir * nbg) <= 256 && ndir * nbg <= MAX_GROUPS),
                "%s: more recurrences than CUs", who);
  B2P_CHECK_ARG(T <= max_T, "%s: T = %lld exceeds the 16-bit step tag", who, (long long)T);
  return xch_prepare(ws, hdr_bytes(B, H, ndir), b2p_gru_mc_workspace(B, H, ndir), st, w);
}

extern "C" int b2p_gru_fwd_mc(const float* gi, const float* whh, const float* bhh, const float* h0, float* out,
                              float* saved, void* workspace, int64_t B, int64_t T, int64_t H, int ndir,
                              b2p_stream_t stream) {
  hipStream_t st = (hipStream_t)stream;
  XchWs w;
  if (int r = mc_prepare("gru_fwd_mc", gi && whh && out && saved, workspace, B, T, INT64_MAX, H, ndir, st, &w))
    return r < 0 ? 0 : r;
  if (H == 256) return launch_fwd<256>(w, (int)B, (int)T, ndir, st, gi, whh, bhh, h0, out, saved);
  if (H == 384) return launch_fwd<384>(w, (int)B, (int)T, ndir, st, gi, whh, bhh, h0, out, saved);
  if (H == 1024) return launch_fwd<1024>(w, (int)B, (int)T, ndir, st, gi, whh, bhh, h0, out, saved);
  return launch_fwd<512>(w, (int)B, (int)T, ndir, st, gi, whh, bhh, h0, out, saved);
}

extern "C" int b2p_gru_bwd_mc(const float* dout, const float* whh, const float* out, const float* saved,
                              const float* h0, float* dgi, float* dgh, float* dh0, void* workspace, int64_t B,
                              int64_t T, int64_t H, int ndir, b2p_stream_t stream) {
  hipStream_t st = (hipStream_t)stream;
  XchWs w;
  if (int r = mc_prepare("gru_bwd_mc", dout && whh && out && saved && dgi && dgh, workspace, B, T, 0xFFFE, H, ndir,
                         st, &w))
    return r < 0 ? 0 : r;
  if (H == 256) return launch_bwd<256>(w, (int)B, (int)T, ndir, st, dout, whh, out, saved, h0, dgi, dgh, dh0);
  if (H == 384) return launch_bwd<384>(w, (int)B, (int)T, ndir, st, dout, whh, out, saved, h0, dgi, dgh, dh0);
  if (H == 1024) return launch_bwd<1024>(w, (int)B, (int)T, ndir, st, dout, whh, out, saved, h0, dgi, dgh, dh0);
  return launch_bwd<512>(w, (int)B, (int)T, ndir, st, dout, whh, out, saved, h0, dgi, dgh, dh0);
}
