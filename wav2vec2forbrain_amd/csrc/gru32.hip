// Persistent exact-fp32 GRU recurrence (nn.GRU semantics, gate order r, z, n) for the fp32-operand
// precision modes (bf16x3, fp32), where the 16-bit persistent forms (csrc/gru16.hip, csrc/grumc.hip) move
// the recorded trajectories too far and the per-step kernels (csrc/gru.hip) cost one launch and one
// W_hh staging per time step. The structure is grumc's: one launch runs the whole time loop, a recurrence
// (direction d, 16 batch rows) is spread over P = H/32 member workgroups, one per CU, each keeping its
// slice of W_hh in registers as MFMA A-operands for the whole launch; the members exchange state every
// step through tagged 8-byte granules, double-buffered by step parity (csrc/gru_xch.h: the same bounded
// polling, fail word and one-XCD check as grumc). What differs is the arithmetic: every W_hh product
// runs on v_mfma_f32_16x16x4_f32 (fp32 operands, fp32 accumulate, bitwise an fmaf chain), a granule is
// {32-bit step tag, one fp32 value}, and the gate math uses the per-step kernels' functions
// (b2p_sigmoid, tanhf). Nothing is rounded to 16 bits anywhere.
//
//   forward : member m owns units [32m, 32m+32). Wave w: 16 of them (w & 1), all three gates, one half of
//             K (w >> 1): 3H/8 A-registers per lane (192 at H = 512). gates^T (3 x 16 x 16) = W_hh[rows]
//             (48 x H/2) . h_{t-1}^T (H/2 x 16) as four fmaf chains of H/4 terms per gate (two
//             accumulators per K half); the upper half's sums go through LDS to the lower half's waves,
//             which apply the gates and publish h_t (32 units x 16 rows = 512 granules per member).
//   backward: partial-dh exchange. Member m multiplies its OWN W_hh rows (r, z, n of its 32 units: 96 x H),
//             transposed, by its own dgh_{s+1} (96 x 16, from LDS: no input exchange) and publishes the
//             partial dh of all H units (wave w: units [wH/4, (w+1)H/4), 24 H/64 A-registers per lane, 192
//             at H = 512); every member then adds the P partials of its own units in member order 0..P-1,
//             in registers, straight from the polled granules. Per step a member reads P * 512 granules,
//             as in the forward (the dgh exchange of grumc would read 3H * 16: three times as many, and
//             more than the sweep's 64 granules per lane at H = 512). Not measured against that form.
// Both are deterministic: fixed chains, fixed member order, every output written once, no atomics on data.
//
// Tensors and layouts are those of b2p_gru_fwd / b2p_gru_bwd: gi, dgi, dgh [B][T][ndir*3H], out
// [B][T][ndir*H], saved [B][T][ndir][4][H] = (r, z, n, W_hn h + b_hn), h0 / dh0 [ndir][B][H]; either form's
// backward can consume either form's saved state.
//
// Co-residency: every member of a launch must be resident, so a launch never has more than
// LAUNCH_BUDGET = 128 workgroups (half the chip's 256 CUs: the frozen weight-gradient GEMMs flushed beside
// the backward keep the rest). ndir * ceil(B/16) * P above that runs as successive launches over
// disjoint batch groups on the same stream, each on its own part of the workspace.
#include "common.h"
#include "gru_dev.h"   // BG, t_of
#include "gru_xch.h"
#include "../../include/b2p_hip.h"

namespace {
constexpr int UPM = 32;            // hidden units per member
constexpr int NTH = XCH_NTH;       // 4 waves
constexpr int MGR = UPM * BG;      // granules one member publishes per step in the forward (512)
constexpr int LAUNCH_BUDGET = 128; // workgroups per launch

__device__ __forceinline__ f32x4 mfma4(float a, float b, const f32x4& c) {
  return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}

// ---- H = 1024 (P = 32 members: at best one whole XCD per recurrence). Everything the size forces sits under
// `H == 1024`, so the 256 / 512 instantiations compile as before.
// A wave's W_hh values are 384 registers per lane in both passes, and a lane has 256 VGPRs + 256 AGPRs. As in
// csrc/grumc.hip ("MFMAs that read W_hh straight from AGPRs"), the MFMAs are inline-asm statements whose A
// operands carry an "a" constraint for the first *_A statements (they stay in AGPRs for the whole launch), "v"
// for the next ones, and the statements from *_L on read theirs from LDS ([fragment][thread] float4: one
// conflict-free ds_read_b128 per four values and step). Nothing inside an asm string is padded by the
// compiler: "s_nop 1" opens every statement (a just-written operand: the accumulators' zeros, a
// v_accvgpr_write of the prologue), an accumulator goes from one MFMA to the next only as the whole C of its
// own chain (no wait), and the last statements of a step end with the wait of their results' way to any other
// reader (8-pass XDL: "s_nop 15" inside the string, so that no compiler copy can come before it).
// The exchange is swept SW1024 granules per lane at a time (sweep_parts: the sweep keeps what it polls in
// registers, and all 64 would be 128 of them), and the members' XCC ids take a stride of their own.
template <int H>
constexpr int ids_stride() { return H == 1024 ? 32 : IDS_PER_GROUP; }
constexpr int SW1024 = 16;
template <int H>
constexpr int sweep_width(int ngr) { return H == 1024 ? SW1024 : ngr; }
// forward: a statement is one float4 chunk of K (4 k-steps x 3 gates, 12 A-values); 32 per step
constexpr int FWD_A = 21;   // chunks 0..20: 252 AGPRs
constexpr int FWD_L = 27;   // chunks 21..26: 72 VGPRs; 27..31 in LDS (15 float4 per thread, 61,440 B)
// backward: a statement is one k-step of 8 output tiles (8 A-values); 48 per step
constexpr int BWD_A = 30;   // statements 0..29: 240 AGPRs (the other 16 are the compiler's: with all 256 taken it
                            // spills loop-invariant addresses to scratch)
constexpr int BWD_L = 30;   // none in VGPRs (16 accumulators and the loop's addresses fill them); 30..47 in LDS
                            // (36 float4 per thread, 147,456 B)
constexpr size_t FRAG_BYTES = (size_t)NTH * 16;
template <int H>
constexpr size_t fwd_lds() { return H == 1024 ? (size_t)BG * (H + 4) * 4 + (32 - FWD_L) * 3 * FRAG_BYTES : 0; }
template <int H>
constexpr size_t bwd_lds() { return H == 1024 ? (48 - BWD_L) * 2 * FRAG_BYTES : 0; }
static_assert(fwd_lds<1024>() + 6144 <= 163840 && bwd_lds<1024>() + 12800 <= 163840, "a CU has 160 KB of LDS");

#define B2P_F32OP "v_mfma_f32_16x16x4_f32"
// c[g] += A[g][j] . b[j] over j = 0..3, gates g = 0..2, in the order of the 256 / 512 loop (j outer, g inner)
#define B2P_MFMA12(NAME, CA, END)                                                                                     \
  __device__ __forceinline__ void NAME(f32x4& c0, f32x4& c1, f32x4& c2, const float* a0, const float* a1,             \
                                       const float* a2, const float* b) {                                             \
    asm("s_nop 1\n\t"                                                                                                 \
        B2P_F32OP " %0, %3, %15, %0\n\t" B2P_F32OP " %1, %7, %15, %1\n\t" B2P_F32OP " %2, %11, %15, %2\n\t"            \
        B2P_F32OP " %0, %4, %16, %0\n\t" B2P_F32OP " %1, %8, %16, %1\n\t" B2P_F32OP " %2, %12, %16, %2\n\t"            \
        B2P_F32OP " %0, %5, %17, %0\n\t" B2P_F32OP " %1, %9, %17, %1\n\t" B2P_F32OP " %2, %13, %17, %2\n\t"            \
        B2P_F32OP " %0, %6, %18, %0\n\t" B2P_F32OP " %1, %10, %18, %1\n\t" B2P_F32OP " %2, %14, %18, %2" END            \
        : "+v"(c0), "+v"(c1), "+v"(c2)                                                                                \
        : CA(a0[0]), CA(a0[1]), CA(a0[2]), CA(a0[3]), CA(a1[0]), CA(a1[1]), CA(a1[2]), CA(a1[3]), CA(a2[0]),          \
          CA(a2[1]), CA(a2[2]), CA(a2[3]), "v"(b[0]), "v"(b[1]), "v"(b[2]), "v"(b[3]));                               \
  }
// c[i] += a[i] . b for 8 output tiles (one k-step)
#define B2P_MFMA8(NAME, CA, END)                                                                                      \
  __device__ __forceinline__ void NAME(f32x4* c, float a0, float a1, float a2, float a3, float a4, float a5,          \
                                       float a6, float a7, float b) {                                                 \
    asm("s_nop 1\n\t"                                                                                                 \
        B2P_F32OP " %0, %8, %16, %0\n\t" B2P_F32OP " %1, %9, %16, %1\n\t" B2P_F32OP " %2, %10, %16, %2\n\t"            \
        B2P_F32OP " %3, %11, %16, %3\n\t" B2P_F32OP " %4, %12, %16, %4\n\t" B2P_F32OP " %5, %13, %16, %5\n\t"          \
        B2P_F32OP " %6, %14, %16, %6\n\t" B2P_F32OP " %7, %15, %16, %7" END                                            \
        : "+v"(c[0]), "+v"(c[1]), "+v"(c[2]), "+v"(c[3]), "+v"(c[4]), "+v"(c[5]), "+v"(c[6]), "+v"(c[7])              \
        : CA(a0), CA(a1), CA(a2), CA(a3), CA(a4), CA(a5), CA(a6), CA(a7), "v"(b));                                    \
  }
B2P_MFMA12(mfma12_a, "a", "")
B2P_MFMA12(mfma12_v, "v", "")
B2P_MFMA12(mfma12_v_last, "v", "\n\ts_nop 15")
B2P_MFMA8(mfma8_a, "a", "")
B2P_MFMA8(mfma8_v, "v", "")
B2P_MFMA8(mfma8_v_last, "v", "\n\ts_nop 15")
#undef B2P_MFMA12
#undef B2P_MFMA8
#undef B2P_F32OP
// prologue: a statement's values are put in their file before the next one's loads are issued (left alone,
// every load of the 384 comes first)
__device__ __forceinline__ void pin_f32(float& x, bool agpr) {
  if (agpr) asm volatile("" : "+a"(x));
  else asm volatile("" : "+v"(x));
}

// ------------------------------------------------------------------------------------------ forward
// exchange slots: [group][2][P * 512] granules. h_s of member m, batch row b, unit u = 16ub + 4lq + i of m sits at
// m*512 + ((4ub + i)*4 + lq)*16 + b: the 64 lanes of one publishing store (fixed ub, i) write 512 contiguous
// bytes (one request per 64-byte line instead of one per lane; the L2's request rate bounds the exchange)
template <int H>
__global__ void __launch_bounds__(NTH, 1) gru32_fwd(const float* __restrict__ gi, const float* __restrict__ whh,
                                                    const float* __restrict__ bhh, const float* __restrict__ h0,
                                                    float* __restrict__ out, float* __restrict__ saved,
                                                    unsigned long long* xch, unsigned long long* ids, int* fail, int B,
                                                    int T, int ndir, int nbg_all, int bg0, int nbg) {
  constexpr int P = H / UPM;
  constexpr int KC = H / 32;                 // float4 chunks of this wave's K half
  constexpr int HP = H + 4;                  // floats per batch row of the h image (16-B stagger)
  constexpr int NGR = P * MGR / NTH;         // granules swept per lane
  constexpr int SW = sweep_width<H>(NGR);    // of them per sweep call
  constexpr int G3 = 3 * H;
  constexpr bool WIDE = H == 1024;           // the h image and the W_hh chunks from FWD_L on in dynamic LDS
  __shared__ __attribute__((aligned(16))) float himg_s[WIDE ? 4 : BG * HP];
  __shared__ __attribute__((aligned(16))) f32x4 red[2 * 3 * 64];   // upper K half's sums: [unit block][gate][lane]
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float* const himg = WIDE ? reinterpret_cast<float*>(smem) : himg_s;
  float4* const wl = reinterpret_cast<float4*>(smem + (size_t)BG * HP * 4);

  int d, bgl, m;
  if (!place(P, ndir * nbg, d, bgl, m, nbg)) return;
  const int bg = bg0 + bgl;
  const int tid = threadIdx.x, w = tid >> 6, l = tid & 63, lr = l & 15, lq = l >> 4;
  const int ub = w & 1, kh = w >> 1;
  const int b = bg * BG + lr;
  const bool bok = b < B;
  const int u0 = m * UPM + ub * 16;            // first unit of this wave's block
  const int j0 = u0 + 4 * lq;                  // this lane's 4 output units
  const int kb = kh * (H / 2);                 // first k of this wave's half
  const float* W = whh + (int64_t)d * G3 * H;
  const int gg = d * nbg_all + bg;
  unsigned long long* xg = xch + (int64_t)gg * 2 * P * MGR;
  bool dead = false;
  const bool local = same_xcd(ids + gg * ids_stride<H>(), P, m, fail, dead);

  // A = W_hh rows of (gate g, unit u0 + lr): k = kb + 16c + 4lq + j sits in wf[g][4c + j], the order in which
  // the h image is read as float4 (any k order does, as long as A and B agree)
  float wf[3][4 * KC];
  if constexpr (WIDE) {   // chunk by chunk: into AGPRs, VGPRs or LDS
#pragma unroll
    for (int c = 0; c < KC; ++c) {
#pragma unroll
      for (int g = 0; g < 3; ++g) {
        const float4 v = *reinterpret_cast<const float4*>(W + (int64_t)(g * H + u0 + lr) * H + kb + 16 * c + 4 * lq);
        if (c >= FWD_L) {
          wl[((c - FWD_L) * 3 + g) * NTH + tid] = v;
        } else {
          wf[g][4 * c] = v.x; wf[g][4 * c + 1] = v.y; wf[g][4 * c + 2] = v.z; wf[g][4 * c + 3] = v.w;
#pragma unroll
          for (int j = 0; j < 4; ++j) pin_f32(wf[g][4 * c + j], c < FWD_A);
        }
      }
      __builtin_amdgcn_sched_barrier(0);
    }
  } else {
#pragma unroll
    for (int g = 0; g < 3; ++g)
#pragma unroll
      for (int c = 0; c < KC; ++c) {
        const float4 v = *reinterpret_cast<const float4*>(W + (int64_t)(g * H + u0 + lr) * H + kb + 16 * c + 4 * lq);
        wf[g][4 * c] = v.x; wf[g][4 * c + 1] = v.y; wf[g][4 * c + 2] = v.z; wf[g][4 * c + 3] = v.w;
      }
  }
  float4 bh[3];
#pragma unroll
  for (int g = 0; g < 3; ++g)
    bh[g] = bhh ? *reinterpret_cast<const float4*>(bhh + (int64_t)d * G3 + g * H + j0) : make_float4(0.f, 0.f, 0.f, 0.f);

  // h_{-1}: h0 (or zeros) into the image, and this lane's own 4 values in registers
  float hp[4] = {0.f, 0.f, 0.f, 0.f};
  for (int i = tid; i < BG * H; i += NTH) {
    const int r = i / H, c = i % H;
    const int bb = bg * BG + r;
    himg[r * HP + c] = (h0 && bb < B) ? h0[((int64_t)d * B + bb) * H + c] : 0.f;
  }
  if (h0 && bok) {
    const float4 v = *reinterpret_cast<const float4*>(h0 + ((int64_t)d * B + b) * H + j0);
    hp[0] = v.x; hp[1] = v.y; hp[2] = v.z; hp[3] = v.w;
  }
  __syncthreads();

  const int64_t gstride = (int64_t)ndir * G3, ostride = (int64_t)ndir * H;
  const bool gate_wave = kh == 0;   // the lower K half's waves add the halves, apply the gates and publish
  auto load_gi = [&](int s, float4 (&g)[3]) {
    const int t = t_of(s, d, T);
    const float* gp = gi + ((int64_t)b * T + t) * gstride + d * G3 + j0;
    if (bok && gate_wave)
#pragma unroll
      for (int q = 0; q < 3; ++q) g[q] = *reinterpret_cast<const float4*>(gp + q * H);
  };
  float4 gc[3];   // this step's input projection (the next step's is loaded into it once consumed)
#pragma unroll
  for (int q = 0; q < 3; ++q) gc[q] = make_float4(0.f, 0.f, 0.f, 0.f);
  load_gi(0, gc);
  for (int s = 0; s < T; ++s) {
    if (s > 0) {   // h_{s-1} of every member: tag s, slot (s-1) & 1. Every wave left the image at the
                   // reduction barrier of step s-1, so one image does.
      const unsigned tag = (unsigned)s;
      sweep_parts<NGR, SW>(xg + ((s - 1) & 1) * P * MGR, [tag](unsigned long long x) { return (unsigned)(x >> 32) == tag; },
                 [&](int q, unsigned long long x) {
                   const int uu = ((q >> 8) & 1) * 16 + ((q >> 4) & 3) * 4 + ((q >> 6) & 3);
                   himg[(q & 15) * HP + (q >> 9) * UPM + uu] = __uint_as_float((unsigned)x);
                 }, fail, dead);
      __syncthreads();
    }
    f32x4 acc[3][2];
#pragma unroll
    for (int g = 0; g < 3; ++g) acc[g][0] = acc[g][1] = f32x4{0.f, 0.f, 0.f, 0.f};
    const float* hrow = himg + lr * HP + kb + 4 * lq;
    if constexpr (WIDE) {
      float4 nb = *reinterpret_cast<const float4*>(hrow);   // h is read one chunk ahead of its MFMAs
#pragma unroll
      for (int c = 0; c < KC; ++c) {
        const float4 hv = nb;
        if (c + 1 < KC) nb = *reinterpret_cast<const float4*>(hrow + 16 * (c + 1));
        const float hk[4] = {hv.x, hv.y, hv.z, hv.w};
        f32x4 &c0 = acc[0][c & 1], &c1 = acc[1][c & 1], &c2 = acc[2][c & 1];
        if (c < FWD_A) mfma12_a(c0, c1, c2, wf[0] + 4 * c, wf[1] + 4 * c, wf[2] + 4 * c, hk);
        else if (c < FWD_L) mfma12_v(c0, c1, c2, wf[0] + 4 * c, wf[1] + 4 * c, wf[2] + 4 * c, hk);
        else {
          const float4* wp = wl + (c - FWD_L) * 3 * NTH + tid;
          const float4 v0 = wp[0], v1 = wp[NTH], v2 = wp[2 * NTH];
          const float w0[4] = {v0.x, v0.y, v0.z, v0.w}, w1[4] = {v1.x, v1.y, v1.z, v1.w};
          const float w2[4] = {v2.x, v2.y, v2.z, v2.w};
          if (c < KC - 2) mfma12_v(c0, c1, c2, w0, w1, w2, hk);
          else mfma12_v_last(c0, c1, c2, w0, w1, w2, hk);   // the last statement of either accumulator set
        }
      }
    } else {
#pragma unroll
      for (int c = 0; c < KC; ++c) {
        const float4 hv = *reinterpret_cast<const float4*>(hrow + 16 * c);
        const float hk[4] = {hv.x, hv.y, hv.z, hv.w};
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
          for (int g = 0; g < 3; ++g) acc[g][c & 1] = mfma4(wf[g][4 * c + j], hk[j], acc[g][c & 1]);
      }
    }
    f32x4 a[3];
#pragma unroll
    for (int g = 0; g < 3; ++g) a[g] = acc[g][0] + acc[g][1];
    if (!gate_wave) {
#pragma unroll
      for (int g = 0; g < 3; ++g) red[(ub * 3 + g) * 64 + l] = a[g];
    }
    __syncthreads();
    if (gate_wave) {
#pragma unroll
      for (int g = 0; g < 3; ++g) a[g] += red[(ub * 3 + g) * 64 + l];
      const float gr[4] = {gc[0].x, gc[0].y, gc[0].z, gc[0].w}, gz[4] = {gc[1].x, gc[1].y, gc[1].z, gc[1].w};
      const float gn[4] = {gc[2].x, gc[2].y, gc[2].z, gc[2].w};
      const float br[4] = {bh[0].x, bh[0].y, bh[0].z, bh[0].w}, bz[4] = {bh[1].x, bh[1].y, bh[1].z, bh[1].w};
      const float bn[4] = {bh[2].x, bh[2].y, bh[2].z, bh[2].w};
      float hh[4], rr[4], zz[4], nn[4], gh[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        rr[i] = b2p_sigmoid(gr[i] + (a[0][i] + br[i]));
        zz[i] = b2p_sigmoid(gz[i] + (a[1][i] + bz[i]));
        gh[i] = a[2][i] + bn[i];
        nn[i] = tanhf(gn[i] + rr[i] * gh[i]);
        hh[i] = bok ? (1.f - zz[i]) * nn[i] + zz[i] * hp[i] : 0.f;
        hp[i] = hh[i];
      }
      // publish h_s FIRST (the other members wait on it), then this step's outputs and the next step's
      // input projection
      if (s + 1 < T) {
        unsigned long long* dst = xg + (s & 1) * P * MGR + m * MGR + (ub * 16 + lq) * 16 + lr;
#pragma unroll
        for (int i = 0; i < 4; ++i) put_granule(dst + i * 64, (unsigned)(s + 1), __float_as_uint(hh[i]), local);
      }
      if (bok) {
        const int t = t_of(s, d, T);
        *reinterpret_cast<float4*>(out + ((int64_t)b * T + t) * ostride + d * H + j0) =
            make_float4(hh[0], hh[1], hh[2], hh[3]);
        float* sv = saved + (((int64_t)b * T + t) * ndir + d) * 4 * H + j0;
        *reinterpret_cast<float4*>(sv) = make_float4(rr[0], rr[1], rr[2], rr[3]);
        *reinterpret_cast<float4*>(sv + H) = make_float4(zz[0], zz[1], zz[2], zz[3]);
        *reinterpret_cast<float4*>(sv + 2 * H) = make_float4(nn[0], nn[1], nn[2], nn[3]);
        *reinterpret_cast<float4*>(sv + 3 * H) = make_float4(gh[0], gh[1], gh[2], gh[3]);
      }
      if (s + 1 < T) load_gi(s + 1, gc);
    }
  }
}

// ----------------------------------------------------------------------------------------- backward
// Processing steps run backwards (s = T-1 .. 0, t = t(s)). For own units j:
//   dh_s = dout[t] + [s < T-1] (z_{s+1} dh_{s+1} + (W^T dgh_{s+1})_j)
//   dn = dh (1-z); dz = dh (h_{s-1} - n); dan = dn (1 - n^2); dar = dan ghn r (1-r); daz = dz z (1-z)
//   dgi = (dar, daz, dan), dgh = (dar, daz, dan r)
// exchange slots: [group][2][P (reader md)][P (writer ms)][512] granules: the partial dh of unit u = 16e + 4lq + i
// of md, batch row b, from ms's gate rows, at (md*P + ms)*512 + ((4e + i)*4 + lq)*16 + b, so that the 64 lanes
// of one publishing store write 512 contiguous bytes (as in the forward). Thread tid (wave w, lane lq, lr)
// therefore owns batch row lr and the units 4lq + w and 16 + 4lq + w of its member.
template <int H>
__global__ void __launch_bounds__(NTH, 1) gru32_bwd(const float* __restrict__ dout, const float* __restrict__ whh,
                                                    const float* __restrict__ out, const float* __restrict__ saved,
                                                    const float* __restrict__ h0, float* __restrict__ dgi,
                                                    float* __restrict__ dgh, float* __restrict__ dh0,
                                                    unsigned long long* xch, unsigned long long* ids, int* fail, int B,
                                                    int T, int ndir, int nbg_all, int bg0, int nbg) {
  constexpr int P = H / UPM;
  constexpr int G3 = 3 * H;
  constexpr int NT = H / 64;                   // 16-unit output tiles per wave
  constexpr int KO = 3 * UPM;                  // own gate rows: k = 32*gate + unit
  constexpr int KC = KO / 16;                  // float4 chunks of k
  constexpr int DP = KO + 4;                   // floats per batch row of the dgh image (16-B stagger)
  constexpr int NGR = P * MGR / NTH;           // granules swept per lane: both elements' P partials
  constexpr int SW = sweep_width<H>(NGR);      // of them per sweep call
  constexpr bool WIDE = H == 1024;             // W^T's statements from BWD_L on in dynamic LDS
  __shared__ __attribute__((aligned(16))) float dimg[2 * BG * DP];   // own dgh of step s in image s & 1
  extern __shared__ __attribute__((aligned(16))) char smem[];
  float4* const wl = reinterpret_cast<float4*>(smem);

  int d, bgl, m;
  if (!place(P, ndir * nbg, d, bgl, m, nbg)) return;
  const int bg = bg0 + bgl;
  const int tid = threadIdx.x, w = tid >> 6, l = tid & 63, lr = l & 15, lq = l >> 4;
  const float* W = whh + (int64_t)d * G3 * H;
  const int gg = d * nbg_all + bg;
  unsigned long long* xg = xch + (int64_t)gg * 2 * P * P * MGR;
  bool dead = false;
  const bool local = same_xcd(ids + gg * ids_stride<H>(), P, m, fail, dead);

  // A = W_hh^T: row = output unit w*H/4 + 16t + lr, k = 16c + 4lq + j (gate k >> 5, own unit k & 31) in
  // wt[t][4c + j]
  float wt[NT][4 * KC];
  if constexpr (WIDE) {   // statement (k-step 4c + j, tiles 8hf .. 8hf + 7) by statement: into AGPRs, VGPRs or LDS
    static_assert(H != 1024 || NT == 16, "two statements of 8 tiles per k-step");
#pragma unroll
    for (int kk = 0; kk < 4 * KC; ++kk)
#pragma unroll
      for (int hf = 0; hf < 2; ++hf) {
        const int st = 2 * kk + hf;
        const int k = 16 * (kk >> 2) + 4 * lq + (kk & 3);
        const float* wp = W + (int64_t)((k >> 5) * H + m * UPM + (k & 31)) * H + w * (H / 4) + lr;
        float v[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) v[i] = wp[16 * (8 * hf + i)];
        if (st >= BWD_L) {
          wl[((st - BWD_L) * 2) * NTH + tid] = make_float4(v[0], v[1], v[2], v[3]);
          wl[((st - BWD_L) * 2 + 1) * NTH + tid] = make_float4(v[4], v[5], v[6], v[7]);
        } else {
#pragma unroll
          for (int i = 0; i < 8; ++i) {
            wt[8 * hf + i][kk] = v[i];
            pin_f32(wt[8 * hf + i][kk], st < BWD_A);
          }
        }
        __builtin_amdgcn_sched_barrier(0);
      }
  } else {
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
      for (int c = 0; c < KC; ++c)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int k = 16 * c + 4 * lq + j;
          wt[t][4 * c + j] = W[(int64_t)((k >> 5) * H + m * UPM + (k & 31)) * H + w * (H / 4) + 16 * t + lr];
        }
  }

  int be[2], ue[2], je[2];
  bool ok[2];
#pragma unroll
  for (int e = 0; e < 2; ++e) {
    be[e] = bg * BG + lr;
    ok[e] = be[e] < B;
    ue[e] = 16 * e + 4 * lq + w;
    je[e] = m * UPM + ue[e];
  }
  float dhn[2] = {0.f, 0.f}, zn[2] = {0.f, 0.f};
  const int64_t gstride = (int64_t)ndir * G3, ostride = (int64_t)ndir * H;

  // partial sums of own units from every member: tag, slot parity -> rec[e], added in member order
  auto gather = [&](int par, unsigned tag, float (&rec)[2]) __attribute__((always_inline)) {
    float r0 = 0.f, r1 = 0.f;   // granule q = 256k + tid: member k >> 1, element k & 1 (adding 0.f is exact)
    sweep_parts<NGR, SW>(xg + ((int64_t)par * P + m) * P * MGR, [tag](unsigned long long x) { return (unsigned)(x >> 32) == tag; },
               [&](int q, unsigned long long x) {
                 const float v = __uint_as_float((unsigned)x);
                 const bool hi = (q >> 8) & 1;
                 r0 += hi ? 0.f : v;
                 r1 += hi ? v : 0.f;
               }, fail, dead);
    rec[0] = r0;
    rec[1] = r1;
  };

  for (int s = T - 1; s >= 0; --s) {
    const int t = t_of(s, d, T);
    const int tp = d == 0 ? t - 1 : t + 1;
    float dv[2], r[2], z[2], n[2], ghn[2], hprev[2];
#pragma unroll
    for (int e = 0; e < 2; ++e) {
      dv[e] = r[e] = z[e] = n[e] = ghn[e] = hprev[e] = 0.f;
      if (ok[e]) {
        dv[e] = dout[((int64_t)be[e] * T + t) * ostride + d * H + je[e]];
        const float* sv = saved + (((int64_t)be[e] * T + t) * ndir + d) * 4 * H + je[e];
        r[e] = sv[0]; z[e] = sv[H]; n[e] = sv[2 * H]; ghn[e] = sv[3 * H];
        if (s > 0) hprev[e] = out[((int64_t)be[e] * T + tp) * ostride + d * H + je[e]];
        else if (h0) hprev[e] = h0[((int64_t)d * B + be[e]) * H + je[e]];
      }
    }
    float rec[2] = {0.f, 0.f};
    if (s < T - 1) gather((s + 1) & 1, (unsigned)(s + 2), rec);
    float* img = dimg + (s & 1) * BG * DP;
#pragma unroll
    for (int e = 0; e < 2; ++e) {
      float dh = s < T - 1 ? rec[e] + zn[e] * dhn[e] : 0.f;
      dh += dv[e];
      const float dn = dh * (1.f - z[e]);
      const float dz = dh * (hprev[e] - n[e]);
      const float dan = dn * (1.f - n[e] * n[e]);
      const float dr = dan * ghn[e];
      const float dar = ok[e] ? dr * r[e] * (1.f - r[e]) : 0.f;
      const float daz = ok[e] ? dz * z[e] * (1.f - z[e]) : 0.f;
      const float dgn = ok[e] ? dan * r[e] : 0.f;
      dhn[e] = ok[e] ? dh : 0.f;
      zn[e] = z[e];
      float* ip = img + lr * DP + ue[e];
      ip[0] = dar; ip[UPM] = daz; ip[2 * UPM] = dgn;
      if (ok[e]) {
        float* gi_o = dgi + ((int64_t)be[e] * T + t) * gstride + d * G3 + je[e];
        float* gh_o = dgh + ((int64_t)be[e] * T + t) * gstride + d * G3 + je[e];
        gi_o[0] = dar; gi_o[H] = daz; gi_o[2 * H] = dan;
        gh_o[0] = dar; gh_o[H] = daz; gh_o[2 * H] = dgn;
      }
    }
    // image s & 1 is next written at step s-2, behind the barrier of step s-1, which no wave reaches
    // before it has read this one
    __syncthreads();
    if (s > 0 || dh0) {   // the step before (or dh0) needs W^T dgh_s
      f32x4 acc[NT];
#pragma unroll
      for (int tt = 0; tt < NT; ++tt) acc[tt] = f32x4{0.f, 0.f, 0.f, 0.f};
      const float* grow = img + lr * DP + 4 * lq;
      if constexpr (WIDE) {
        float4 n0 = make_float4(0.f, 0.f, 0.f, 0.f), n1 = n0;
#pragma unroll
        for (int c = 0; c < KC; ++c) {
          const float4 gv = *reinterpret_cast<const float4*>(grow + 16 * c);
          const float gk[4] = {gv.x, gv.y, gv.z, gv.w};
#pragma unroll
          for (int jj = 0; jj < 4; ++jj)
#pragma unroll
            for (int hf = 0; hf < 2; ++hf) {
              const int kk = 4 * c + jj, st = 2 * kk + hf;
              f32x4* a = acc + 8 * hf;
              float (*x)[4 * KC] = wt + 8 * hf;
              // an LDS statement's values are read one statement ahead, and no further (the fence below): read
              // all at once they would be 80 live registers
              const float4 v0 = n0, v1 = n1;
              if (st + 1 >= BWD_L && st + 1 < 8 * KC) {
                n0 = wl[(st + 1 - BWD_L) * 2 * NTH + tid];
                n1 = wl[((st + 1 - BWD_L) * 2 + 1) * NTH + tid];
              }
              if (st < BWD_A)
                mfma8_a(a, x[0][kk], x[1][kk], x[2][kk], x[3][kk], x[4][kk], x[5][kk], x[6][kk], x[7][kk], gk[jj]);
              else if (st < BWD_L)
                mfma8_v(a, x[0][kk], x[1][kk], x[2][kk], x[3][kk], x[4][kk], x[5][kk], x[6][kk], x[7][kk], gk[jj]);
              else if (st < 8 * KC - 2)
                mfma8_v(a, v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z, v1.w, gk[jj]);
              else   // either half's last statement
                mfma8_v_last(a, v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z, v1.w, gk[jj]);
              if (st + 1 >= BWD_L) __builtin_amdgcn_sched_barrier(0);
            }
        }
      } else {
#pragma unroll
        for (int c = 0; c < KC; ++c) {
          const float4 gv = *reinterpret_cast<const float4*>(grow + 16 * c);
          const float gk[4] = {gv.x, gv.y, gv.z, gv.w};
#pragma unroll
          for (int jj = 0; jj < 4; ++jj)
#pragma unroll
            for (int tt = 0; tt < NT; ++tt) acc[tt] = mfma4(wt[tt][4 * c + jj], gk[jj], acc[tt]);
        }
      }
      unsigned long long* slot = xg + (int64_t)(s & 1) * P * P * MGR;
      const unsigned tag = (unsigned)(s + 1);
      if constexpr (WIDE) {
        // tile 0's address made opaque once per step, the others a constant away from it (the same addresses
        // as below): built from the loop's invariants, all 16 tiles' 64-bit addresses stay live across the step
        unsigned long long* base = slot + ((int64_t)(w * (H / 128)) * P + m) * MGR + lq * 16 + lr;
        asm volatile("" : "+v"(base));
#pragma unroll
        for (int tt = 0; tt < NT; ++tt) {
          unsigned long long* dst = base + (int64_t)(tt >> 1) * P * MGR + (tt & 1) * 256;
#pragma unroll
          for (int i = 0; i < 4; ++i) put_granule(dst + i * 64, tag, __float_as_uint(acc[tt][i]), local);
        }
      } else {
#pragma unroll
        for (int tt = 0; tt < NT; ++tt) {
          const int ju = w * (H / 4) + 16 * tt + 4 * lq;   // first of this lane's 4 output units (one member's)
          unsigned long long* dst = slot + ((int64_t)(ju >> 5) * P + m) * MGR + ((tt & 1) * 16 + lq) * 16 + lr;
#pragma unroll
          for (int i = 0; i < 4; ++i) put_granule(dst + i * 64, tag, __float_as_uint(acc[tt][i]), local);
        }
      }
    }
  }
  if (dh0) {   // dh0 = W^T dgh_0 + z_0 dh_0
    float rec[2];
    gather(0, 1u, rec);
#pragma unroll
    for (int e = 0; e < 2; ++e)
      if (ok[e]) dh0[((int64_t)d * B + be[e]) * H + je[e]] = rec[e] + zn[e] * dhn[e];
  }
}

bool supported32(int64_t H) { return H == 256 || H == 512 || H == 1024; }
int64_t ngroups_all(int64_t B, int ndir) { return (int64_t)ndir * ((B + BG - 1) / BG); }
// workspace: [fail word block 16 B][ids: groups x 16 (H = 1024: 32) x 8 B][exchange slots]
int64_t hdr_bytes(int64_t B, int64_t H, int ndir) {
  return 16 + ngroups_all(B, ndir) * (H == 1024 ? ids_stride<1024>() : ids_stride<512>()) * 8;
}
int64_t fwd_bytes(int64_t B, int64_t H, int ndir) {
  return hdr_bytes(B, H, ndir) + ngroups_all(B, ndir) * 2 * (H / UPM) * MGR * 8;
}
int64_t bwd_bytes(int64_t B, int64_t H, int ndir) {
  return hdr_bytes(B, H, ndir) + ngroups_all(B, ndir) * 2 * (H / UPM) * (H / UPM) * MGR * 8;
}

// batch groups per launch: every direction of a batch group in the same launch, at most LAUNCH_BUDGET
// workgroups (grid_blocks rounds up to 8 recurrences)
int groups_per_launch(int64_t H, int ndir) {
  const int P = (int)(H / UPM);
  int nb = LAUNCH_BUDGET / P / ndir;
  return nb < 1 ? 1 : nb;
}

template <typename K, typename... A>
int launch_chunks(K kernel, size_t lds, int64_t B, int64_t H, int ndir, hipStream_t st, A... args) {
  const int P = (int)(H / UPM);
  const int nbg_all = (int)((B + BG - 1) / BG), step = groups_per_launch(H, ndir);
  for (int bg0 = 0; bg0 < nbg_all; bg0 += step) {
    const int nbg = nbg_all - bg0 < step ? nbg_all - bg0 : step;
    hipLaunchKernelGGL(kernel, dim3(grid_blocks(P, ndir * nbg)), dim3(NTH), lds, st, args..., nbg_all, bg0, nbg);
    B2P_CHECK_LAUNCH();
  }
  return 0;
}

// the H = 1024 kernels' dynamic LDS is above the 64 KB a launch gets unasked (once per kernel, as grumc's launch_mc)
int wide_lds(bool& done, const void* kernel, size_t lds) {
  if (!done) {
    B2P_CHECK_HIP(hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    done = true;
  }
  return 0;
}
}  // namespace

extern "C" int b2p_gru32_supported(int64_t H) { return supported32(H) ? 1 : 0; }

extern "C" int64_t b2p_gru32_workspace(int64_t B, int64_t H, int ndir) {
  if (!supported32(H) || (ndir != 1 && ndir != 2)) return 0;
  return bwd_bytes(B < 0 ? 0 : B, H, ndir);   // sized for the backward (P times the forward's slots)
}

// The checks of both entry points, then the fail word, the ids and every polled slot (zero_bytes) zeroed before the
// launches (a node of a captured graph) and the workspace carved. 0 go on, 1 / 2 error set, -1 nothing to do.
static int prepare32(const char* who, bool pointers, void* ws, int64_t zero_bytes, int64_t B, int64_t T, int64_t H,
                     int ndir, hipStream_t st, XchWs* w) {
  if (int r = xch_check_args(who, pointers, supported32(H), H, "256, 512 or 1024", ndir, ws, B, T)) return r;
  B2P_CHECK_ARG(B < (1ll << 24) && T < (1ll << 30), "%s: B or T out of range", who);
  return xch_prepare(ws, hdr_bytes(B, H, ndir), zero_bytes, st, w);
}

extern "C" int b2p_gru_fwd32(const float* gi, const float* whh, const float* bhh, const float* h0, float* out,
                             float* saved, void* workspace, int64_t B, int64_t T, int64_t H, int ndir,
                             b2p_stream_t stream) {
  hipStream_t st = (hipStream_t)stream;
  XchWs w;
  if (int r = prepare32("gru32 fwd", gi && whh && out && saved, workspace, fwd_bytes(B, H, ndir), B, T, H, ndir, st, &w))
    return r < 0 ? 0 : r;
  if (H == 1024) {
    static bool attr = false;
    if (int r = wide_lds(attr, (const void*)gru32_fwd<1024>, fwd_lds<1024>())) return r;
    return launch_chunks(gru32_fwd<1024>, fwd_lds<1024>(), B, H, ndir, st, gi, whh, bhh, h0, out, saved, w.xch, w.ids,
                         w.fail, (int)B, (int)T, ndir);
  }
  return launch_chunks(H == 256 ? gru32_fwd<256> : gru32_fwd<512>, 0, B, H, ndir, st, gi, whh, bhh, h0, out, saved,
                       w.xch, w.ids, w.fail, (int)B, (int)T, ndir);
}

extern "C" int b2p_gru_bwd32(const float* dout, const float* whh, const float* out, const float* saved,
                             const float* h0, float* dgi, float* dgh, float* dh0, void* workspace, int64_t B,
                             int64_t T, int64_t H, int ndir, b2p_stream_t stream) {
  hipStream_t st = (hipStream_t)stream;
  XchWs w;
  if (int r = prepare32("gru32 bwd", dout && whh && out && saved && dgi && dgh, workspace, bwd_bytes(B, H, ndir), B, T,
                        H, ndir, st, &w))
    return r < 0 ? 0 : r;
  if (H == 1024) {
    static bool attr = false;
    if (int r = wide_lds(attr, (const void*)gru32_bwd<1024>, bwd_lds<1024>())) return r;
    return launch_chunks(gru32_bwd<1024>, bwd_lds<1024>(), B, H, ndir, st, dout, whh, out, saved, h0, dgi, dgh, dh0,
                         w.xch, w.ids, w.fail, (int)B, (int)T, ndir);
  }
  return launch_chunks(H == 256 ? gru32_bwd<256> : gru32_bwd<512>, 0, B, H, ndir, st, dout, whh, out, saved, h0, dgi,
                       dgh, dh0, w.xch, w.ids, w.fail, (int)B, (int)T, ndir);
}
