// gemm16 kernel templates (shared by gemm16.hip and the instantiation units gemm16_{nt,nt16,misc}.hip;
// see gemm16.hip for the design notes). build_lib.py tracks this file as a dependency of its includers.
#pragma once
#include "common.h"
#include "../../include/b2p_hip.h"
#include "gemm_epi.h"
#include <stdio.h>
#include <stdlib.h>
#include <type_traits>



namespace {

constexpr int NT16 = 256;
constexpr int TILE = 128;


__device__ __attribute__((aligned(16))) uint32_t g_zero_page[8];   // zero-initialised

typedef __attribute__((address_space(3))) void lds_t;
typedef short s16x4 __attribute__((ext_vector_type(4)));
typedef _Float16 f16x8g __attribute__((ext_vector_type(8)));

// One 16-B-per-lane LDS-DMA (global_load_lds_dwordx4: 1 KB per wave at the wave-uniform LDS address dst,
// lane L at dst + 16 L). Issued as inline asm (M0 written and restored inside the statement), so the
// compiler does not see a pending LDS write: with the builtin it made every ds_read_b64_tr_b16 fragment
// read (an intrinsic whose LDS access it cannot disambiguate) wait vmcnt(0), draining the DMA of the
// next K-tile before each read phase of the m/n-contiguous (weight-gradient, backward-data) layouts.
// Every read of DMA'd data is ordered by the kernels' own counted vmcnt waits and barriers; the compiler's
// waits for its own loads stay correct (an asm DMA issued before such a load retires before it, one
// issued after it only makes the compiler's count conservative).
// dst: a generic pointer into the kernel's __shared__ array; the low 32 bits of a generic LDS address are
// the LDS byte offset (no address-space cast, whose null check cost registers in the loop)
__device__ __forceinline__ void glds16(const void* src, const char* dst) {
  const uint32_t lds = __builtin_amdgcn_readfirstlane((uint32_t)(uintptr_t)dst);
  uint32_t keep;
  asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
               : "=&s"(keep)
               : "v"(src), "s"(lds)
               : "memory");
}

template <int N>
__device__ __forceinline__ void wait_vm() {
  asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}

// swizzle of a k-contiguous image with 2*KT-byte rows (slot = chunk ^ swz_k(row)); both make a
// 16x32 ds_read_b128 fragment read conflict-free (each 16-lane group covers all 64 banks once)
template <int KT>
__device__ __forceinline__ int swz_k(int r) {
  if constexpr (KT == 64) return (r >> 1) & 7;
  else return ((r >> 3) & 1) << 1;
}
// swizzle of an mn-contiguous image with 256-B rows (128 bf16), for ds_read_b64_tr_b16
__device__ __forceinline__ int swz_t(int r) { return ((r & 3) << 2) | ((r >> 2) & 3); }

// per-lane source state of one ROWS x KT operand tile (NWAVES waves issue it together)
template <int ROWS, int KT, bool INNER_K, bool CONV, int NWAVES>
struct Src {
  static constexpr int NJ = ROWS * KT * 2 / 1024;   // glds wave-instructions per tile (all waves)
  static constexpr int NI = NJ / NWAVES;            // per wave
  static constexpr int RPI = 1024 / (2 * KT);       // INNER_K: rows per instruction
  static constexpr int LPR = KT / 8;                // INNER_K: lanes per row
  static constexpr int CPR = ROWS / 8;              // !INNER_K: 16-B chunks per k-row
  static constexpr int KPI = 64 / CPR;              // !INNER_K: k-rows per instruction
  static_assert(NI * NWAVES == NJ && NI >= 1, "tile not divisible over the waves");
  const uint16_t* p[NI];
  int kofs[NI];
  bool ok[NI];
  int64_t rowoff[NI];
  int frame0[NI], tap[NI], ch[NI];
  const uint16_t* base;
  int64_t ld;
  int T_in, Cg;

  __device__ __forceinline__ void init(const b2p_operand& o, int z1, int z2, int wave, int lane, int mn0, int MN,
                                       int kbeg) {
    const int64_t i1 = o.gather1 ? o.gather1[z1] : (int64_t)z1;
    base = static_cast<const uint16_t*>(o.ptr) + i1 * o.bs1 + (int64_t)z2 * o.bs2;
    ld = o.ld;
#pragma unroll
    for (int i = 0; i < NI; ++i) {
      const int j = wave * NI + i;
      if constexpr (INNER_K) {
        const int r = RPI * j + lane / LPR;
        const int c = (lane % LPR) ^ swz_k<KT>(r);
        const int row = mn0 + r;
        ok[i] = row < MN;
        kofs[i] = 8 * c;
        if constexpr (CONV) {
          const int T_out = o.conv_T_out;
          const int rr = ok[i] ? row : 0;
          const int b = rr / T_out, t = rr - b * T_out;
          rowoff[i] = (int64_t)b * o.conv_sample_stride;
          frame0[i] = t * o.conv_stride - o.conv_pad;
          const int k = kbeg + 8 * c;
          tap[i] = k / o.conv_Cg;
          ch[i] = k - tap[i] * o.conv_Cg;
          p[i] = base;
        } else {
          p[i] = base + (int64_t)(ok[i] ? row : 0) * ld + kbeg + 8 * c;
        }
      } else {
        const int r = KPI * j + lane / CPR;
        const int c = (lane % CPR) ^ swz_t(r);
        const int mn = mn0 + 8 * c;
        ok[i] = mn < MN;
        kofs[i] = r;
        p[i] = base + (int64_t)(kbeg + r) * ld + (ok[i] ? mn : 0);
      }
    }
    if constexpr (CONV) {
      T_in = o.conv_T_in;
      Cg = o.conv_Cg;
    }
  }

  // this wave's NI glds for the tile starting at k0 into the operand image `img`
  __device__ __forceinline__ void issue(char* img, int wave, int k0, int K) {
#pragma unroll
    for (int i = 0; i < NI; ++i) {
      const void* src;
      if constexpr (INNER_K && CONV) {
        const int f = frame0[i] + tap[i];
        const bool v = ok[i] && (k0 + kofs[i] < K) && f >= 0 && f < T_in;
        src = v ? (const void*)(base + rowoff[i] + (int64_t)f * ld + ch[i]) : (const void*)g_zero_page;
        ch[i] += KT;
        while (ch[i] >= Cg) { ch[i] -= Cg; ++tap[i]; }
      } else {
        const bool v = ok[i] && (k0 + kofs[i] < K);
        src = v ? (const void*)p[i] : (const void*)g_zero_page;
        p[i] += INNER_K ? (int64_t)KT : (int64_t)KT * ld;
      }
      glds16(src, img + (wave * NI + i) * 1024);
    }
  }
};

constexpr uint32_t OOB = 0xFFFFFFF0u;   // byte offset past every resource's num_records

typedef __amdgpu_buffer_rsrc_t rsrc16_t;
__device__ __forceinline__ rsrc16_t mkres(const void* p, uint64_t bytes) {
  const uint32_t n = bytes >= (uint64_t)OOB ? OOB : (uint32_t)bytes;
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p), 0, p ? n : 0u, 0x00020000);
}

// Buffer-resource operand source of the 256-column (ping-pong) kernels: the batch member's operand matrix
// is a raw buffer resource (4 SGPRs) and each lane keeps one 32-bit byte offset per LDS-DMA instruction
// (buffer_load_dwordx4 ... offen lds). Rows outside the operand get an offset past the resource's extent, so
// the hardware returns zeros for them: no zero page, no per-issue selects, a quarter of the per-lane state
// of Src (64-bit pointers, k offsets, row masks). A k-contiguous operand's K tail (k >= K inside a row)
// is masked per lane in the last K-tile only. The host keeps every operand extent below 2^30 bytes
// (b2p_gemm16_launch), so an out-of-range offset stays out of range as it advances.
constexpr uint32_t SRC_OOB = 0x80000000u;
__device__ __forceinline__ void blds16(uint32_t voff, rsrc16_t rs, const char* dst) {
  const uint32_t lds = __builtin_amdgcn_readfirstlane((uint32_t)(uintptr_t)dst);
  uint32_t keep;
  asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %3\n\ts_nop 0\n\tbuffer_load_dwordx4 %1, %2, 0 offen lds\n\ts_mov_b32 m0, %0"
               : "=&s"(keep)
               : "v"(voff), "s"(rs), "s"(lds)
               : "memory");
}
// QM (quarter map, 256-row k-contiguous images, 8 waves x 4 instructions): a wave's instructions 0-1
// load quarter 0 of the image and 2-3 quarter 1, so a quarter can be issued (and waited for) on its own.
// QM 1 (A): quarter h = rows {64h .. 64h+63, 128+64h .. 128+64h+63} (the 64-row halves mi of both wave
// groups' row blocks); QM 2 (B): quarter h = rows {64c + 32h .. 64c + 32h + 31 : c = 0..3} (the 32-column
// halves nj of the four wave columns). QM 0: wave w loads rows 32 w .. 32 w + 31 (instructions 4 w .. 4 w + 3).
template <int QM>
__device__ __forceinline__ int srcb_j(int wave, int i, int NI) {
  if constexpr (QM == 0) {
    return wave * NI + i;
  } else {
    const int idx = 2 * wave + (i & 1), h = i >> 1;
    if constexpr (QM == 1) return (idx < 8 ? idx : idx + 8) + 8 * h;
    else return 8 * (idx >> 2) + 4 * h + (idx & 3);
  }
}
template <int ROWS, int KT, bool INNER_K, int NWAVES, int QM = 0>
struct SrcB {
  static constexpr int NJ = ROWS * KT * 2 / 1024;   // LDS-DMA wave-instructions per tile (all waves)
  static constexpr int NI = NJ / NWAVES;            // per wave
  static constexpr int RPI = 1024 / (2 * KT);       // INNER_K: rows per instruction
  static constexpr int LPR = KT / 8;                // INNER_K: lanes per row
  static constexpr int CPR = ROWS / 8;              // !INNER_K: 16-B chunks per k-row
  static constexpr int KPI = 64 / CPR;              // !INNER_K: k-rows per instruction
  static_assert(NI * NWAVES == NJ && NI >= 1, "tile not divisible over the waves");
  static_assert(QM == 0 || (ROWS == 256 && KT == 64 && INNER_K && NWAVES == 8), "quarter map: 256 x 64 k-contiguous");
  rsrc16_t rs;
  uint32_t off[NI];
  uint32_t step;

  __device__ __forceinline__ void init(const b2p_operand& o, int z1, int z2, int wave, int lane, int mn0, int MN, int K,
                                       int kbeg) {
    const int64_t i1 = o.gather1 ? o.gather1[z1] : (int64_t)z1;
    const uint16_t* base = static_cast<const uint16_t*>(o.ptr) + i1 * o.bs1 + (int64_t)z2 * o.bs2;
    const int64_t ld = o.ld;
    const uint64_t ext = INNER_K ? ((uint64_t)(MN - 1) * ld + K) * 2 : ((uint64_t)(K - 1) * ld + MN) * 2;
    rs = mkres(base, ext);
    step = INNER_K ? 2u * KT : (uint32_t)(2 * KT * ld);
#pragma unroll
    for (int i = 0; i < NI; ++i) {
      const int j = srcb_j<QM>(wave, i, NI);
      if constexpr (INNER_K) {
        const int r = RPI * j + lane / LPR;
        const int c = (lane % LPR) ^ swz_k<KT>(r);
        const int row = mn0 + r;
        off[i] = row < MN ? (uint32_t)(((int64_t)row * ld + kbeg + 8 * c) * 2) : SRC_OOB;
      } else {
        const int r = KPI * j + lane / CPR;
        const int c = (lane % CPR) ^ swz_t(r);
        const int mn = mn0 + 8 * c;
        off[i] = mn < MN ? (uint32_t)(((int64_t)(kbeg + r) * ld + mn) * 2) : SRC_OOB;   // k-rows >= K: past the extent
      }
    }
  }

  // this wave's DMAs I0 .. I1-1 of the K-tile starting at k0 into the operand image img
  template <int I0 = 0, int I1 = NI>
  __device__ __forceinline__ void issue(const char* img, int wave, int lane, int k0, int K) {
    const bool tail = INNER_K && k0 + KT > K;   // wave-uniform
#pragma unroll
    for (int i = I0; i < I1; ++i) {
      const int j = srcb_j<QM>(wave, i, NI);
      uint32_t v = off[i];
      if (tail) {
        const int c = (lane % LPR) ^ swz_k<KT>(RPI * j + lane / LPR);
        if (k0 + 8 * c >= K) v = SRC_OOB;
      }
      blds16(v, rs, img + j * 1024);
      off[i] += step;
    }
  }
  // quarter h (QM != 0): instructions 2h, 2h+1
  template <int H>
  __device__ __forceinline__ void issue_q(const char* img, int wave, int lane, int k0, int K) {
    issue<2 * H, 2 * H + 2>(img, wave, lane, k0, K);
  }
};

// fragment reads ------------------------------------------------------------------------------
// k-contiguous image: rows row0 .. row0+15 (lane & 15) x k = 32*kk + 8*(lane>>4) .. +7
template <int KT>
__device__ __forceinline__ bf16x8 frag_k(const char* img, int row0, int kk, int lane) {
  const int r = row0 + (lane & 15);
  const int c = (4 * kk + (lane >> 4)) ^ swz_k<KT>(r);
  return *reinterpret_cast<const bf16x8*>(img + r * (2 * KT) + c * 16);
}
// mn-contiguous image (ROWS mn-values per k-row): columns col0 .. col0+15 (lane & 15) x
// k = 32*kk + 8*(lane>>4) .. +7
template <int ROWS>
__device__ __forceinline__ bf16x8 frag_t(const char* img, int col0, int kk, int lane) {
  const int g = lane >> 4, q = (lane & 15) >> 2, p = lane & 3;
  const int chunk = (col0 >> 3) + (p >> 1);
  s16x4 h[2];
#pragma unroll
  for (int hh = 0; hh < 2; ++hh) {
    const int row = 32 * kk + 8 * g + 4 * hh + q;
    const char* a = img + row * (2 * ROWS) + ((chunk ^ swz_t(row)) << 4) + 8 * (p & 1);
    h[hh] = __builtin_amdgcn_ds_read_tr16_b64_v4i16((__attribute__((address_space(3))) s16x4*)(a));
  }
  typedef short s16x8 __attribute__((ext_vector_type(8)));
  s16x8 v = {h[0][0], h[0][1], h[0][2], h[0][3], h[1][0], h[1][1], h[1][2], h[1][3]};
  return __builtin_bit_cast(bf16x8, v);
}

// ------------------------------------------------------------------------------------------------
// Register epilogue. The MFMAs run with the operand roles swapped (A-operand = the B fragment,
// B-operand = the A fragment), so each 16x16 accumulator tile is the TRANSPOSE of the output
// block: lane l holds D[m][n .. n+3] with m = row0 + (l & 15), n = col0 + 4 (l >> 4) — four
// consecutive output columns of one row. The epilogue then works and stores straight from the
// accumulators: 16-B vector stores, 64 contiguous bytes per row per wave instruction (fp32 images: one
// column tile per store; 16-bit images: two, after a lane-group swap of the packed values, or 8-B stores of
// one where the launch's alignment does not allow 16 B), no LDS staging, no barrier, no cross-lane traffic
// (except that swap and the fused column sums).
//
// Every access goes through a raw buffer resource: an element outside the matrix gets the offset
// OOB (past num_records), so its load returns 0 and its store is dropped by the hardware — loads and
// stores stay unconditional (straight-line code, exact vmcnt counting). The per-element operands
// (C for beta, aux, residual) of row tile i+1 are loaded BEFORE the stores of row tile i: vmcnt counts
// loads and stores together in issue order, so a load issued after a store would wait for that store
// to reach memory (the round-3 epilogue's per-pass vmcnt(0): 34.5k of an 80k-cycle 256x256 tile).
//
// The epilogue's content is a compile-time kind (bit set below), chosen on the host per launch; a
// launch whose combination has no instantiation runs EK_RUNTIME (the same code with the bits as
// uniform runtime branches, ea.rk), and a launch without 16-B vector accesses the GENERIC kind
// (epilogue_store4 per element group, out of line).
constexpr uint32_t EK_BETA = 1u << 0, EK_BIAS = 1u << 1, EK_PRE32 = 1u << 2, EK_PRE16 = 1u << 3, EK_ACT = 1u << 4,
                   EK_DROP = 1u << 5, EK_ABWD = 1u << 6, EK_AUX16 = 1u << 7, EK_RES = 1u << 8, EK_C32 = 1u << 9,
                   EK_C16 = 1u << 10, EK_C16H = 1u << 11, EK_CSUM = 1u << 12, EK_SLAB = 1u << 13, EK_C16B = 1u << 14,
                   EK_RUNTIME = 1u << 30, EK_GENERIC = 1u << 31;

// the LayerDrop gate of batch member z1: a batched launch of several layers' weight gradients carries
// one gate per member (b2p_set_gate_batch), every other launch the issuing layer's (b2p_set_gate). The
// RUNTIME / GENERIC kinds (at the VGPR limit) read the launch gate only; the host refuses per-member
// gates for them (b2p_gemm16_launch).
template <uint32_t EK>
__device__ __forceinline__ const int32_t* gemm_gate(const EpiArgs& ea, int z1) {
  if constexpr (EK == EK_RUNTIME || EK == EK_GENERIC) return ea.gate;
  else return ea.gates ? reinterpret_cast<const int32_t*>(ea.gates[z1]) : ea.gate;
}
__device__ __forceinline__ float4 bld16(rsrc16_t r, uint32_t off) {
  return __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(r, off, 0, 0));
}
__device__ __forceinline__ uint2 bld8(rsrc16_t r, uint32_t off) {
  return __builtin_bit_cast(uint2, __builtin_amdgcn_raw_buffer_load_b64(r, off, 0, 0));
}
__device__ __forceinline__ void bst16(rsrc16_t r, uint32_t off, float4 v) {
  __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(__attribute__((ext_vector_type(4))) unsigned, v), r, off, 0, 0);
}
// write-through (sc1) 16-B store / sc1 load: the split-K slabs another workgroup sums in this launch
// (cdna_hip_programming.md Guideline 16, R1: no release fence needed, every reader load sc1)
__device__ __forceinline__ void bst16_wt(rsrc16_t r, uint32_t off, float4 v) {
  __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(__attribute__((ext_vector_type(4))) unsigned, v), r, off, 0, 16);
}
__device__ __forceinline__ float4 bld16_sc1(rsrc16_t r, uint32_t off) {
  return __builtin_bit_cast(float4, __builtin_amdgcn_raw_buffer_load_b128(r, off, 0, 16));
}
__device__ __forceinline__ void bst16u(rsrc16_t r, uint32_t off, uint4 v) {
  __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(__attribute__((ext_vector_type(4))) unsigned, v), r, off, 0, 0);
}
__device__ __forceinline__ void bst8(rsrc16_t r, uint32_t off, uint2 v) {
  __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(__attribute__((ext_vector_type(2))) unsigned, v), r, off, 0, 0);
}
__device__ __forceinline__ float4 bf16x4_to_f4(uint2 h) {
  return make_float4(b2p_bf16_to_f32((uint16_t)(h.x & 0xffffu)), b2p_bf16_to_f32((uint16_t)(h.x >> 16)),
                     b2p_bf16_to_f32((uint16_t)(h.y & 0xffffu)), b2p_bf16_to_f32((uint16_t)(h.y >> 16)));
}
// GENERIC kind: the accumulators go through LDS (the K loop's buffers, free after one barrier) two row
// tiles at a time, 68-float rows (conflict-free float4 writes), and come back as 4 consecutive columns per
// lane for a rolled loop of the runtime-flag epilogue_store4: an unrolled loop over the accumulators with
// that body inline made the compiler index them dynamically (scratch), an out-of-line call copied the
// argument block to scratch.
constexpr int GEN_ROWS = 32, GEN_LD = 68;
constexpr int gen_lds_bytes(int nwaves) { return nwaves * GEN_ROWS * GEN_LD * 4; }

// The wave's accumulators acc[MI][4]: row tile i, column tile j (16 x 16 each) of the wave tile at
// (mrow0, ncol0). slab: split-K partial slab of this (z, slice) (EK_SLAB).
template <uint32_t EK, int MI, int NJT = 4>
__device__ __forceinline__ void reg_epilogue(const EpiArgs& ea, const b2p_gemm_desc& d, f32x4 (&acc)[MI][NJT], int z,
                                             int z1, int z2, int mrow0, int ncol0, int lane, float* slab,
                                             char* smem) {
  const int M = (int)d.M, N = (int)d.N;
  const int rl = lane & 15, cq = 4 * (lane >> 4);
  const b2p_epilogue& e = ea.e;
  auto store_slab = [&]() __attribute__((always_inline)) {
    const rsrc16_t rs = mkres(slab, (uint64_t)M * N * 4);
#pragma unroll
    for (int i = 0; i < MI; ++i) {
      const int m = mrow0 + 16 * i + rl;
#pragma unroll
      for (int j = 0; j < NJT; ++j) {
        const int n = ncol0 + 16 * j + cq;
        // N % 4 != 0: element-wise (unaligned rows)
        if ((N & 3) == 0 || m >= M || n >= N) {
          const uint32_t off = (m < M && n < N) ? (uint32_t)(((int64_t)m * N + n) * 4) : OOB;
          const float4 v = make_float4(acc[i][j][0], acc[i][j][1], acc[i][j][2], acc[i][j][3]);
          if (ea.tile_ctr) bst16_wt(rs, off, v);   // summed by another workgroup in this launch
          else bst16(rs, off, v);
        } else {
          for (int q = 0; q < 4 && n + q < N; ++q) slab[(int64_t)m * N + n + q] = acc[i][j][q];
        }
      }
    }
  };
  if constexpr ((EK & EK_GENERIC) != 0) {
    static_assert(NJT == 4, "GENERIC epilogue: 64 columns per wave");
    if (slab) {   // split-K partials (a kind-less launch: e.g. an fp16 NN / TN layout)
      store_slab();
      return;
    }
    static_assert(MI % 2 == 0, "GENERIC epilogue: an even number of row tiles per wave");
    float* stg = reinterpret_cast<float*>(smem) + (threadIdx.x >> 6) * (GEN_ROWS * GEN_LD);
    __syncthreads();   // every wave is done reading the K loop's operand images
    // lane -> 4 columns (lane & 15) of rows (lane >> 4) + 4 t: the column group is fixed per lane
    const int c4 = 4 * (lane & 15), r0 = lane >> 4;
#pragma unroll
    for (int h = 0; h < MI / 2; ++h) {
      float4 cs = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
          *reinterpret_cast<float4*>(stg + (16 * i + rl) * GEN_LD + 16 * j + cq) =
              make_float4(acc[2 * h + i][j][0], acc[2 * h + i][j][1], acc[2 * h + i][j][2], acc[2 * h + i][j][3]);
      __builtin_amdgcn_wave_barrier();
#pragma unroll 1
      for (int r = r0; r < GEN_ROWS; r += 4) {
        const float4 v = *reinterpret_cast<const float4*>(stg + r * GEN_LD + c4);
        const float4 f = epilogue_store4(ea, z, z1, z2, mrow0 + 32 * h + r, ncol0 + c4, v);
        cs.x += f.x; cs.y += f.y; cs.z += f.z; cs.w += f.w;
      }
      __builtin_amdgcn_wave_barrier();
      if (e.colsum_part) {   // the column sums of these 32 rows -> partial row (mrow0 + 32 h) / 32
        const int nprow = (M + 31) / 32, prow = mrow0 / 32 + h;
#pragma unroll
        for (int o = 16; o < 64; o <<= 1) {
          cs.x += __shfl_xor(cs.x, o, 64); cs.y += __shfl_xor(cs.y, o, 64);
          cs.z += __shfl_xor(cs.z, o, 64); cs.w += __shfl_xor(cs.w, o, 64);
        }
        const int n = ncol0 + c4;
        if (r0 == 0 && n < N && prow < nprow) *reinterpret_cast<float4*>(e.colsum_part + (int64_t)prow * N + n) = cs;
      }
    }
    return;
  } else if constexpr ((EK & EK_SLAB) != 0) {
    store_slab();
    return;
  } else {
    if constexpr ((EK & EK_RUNTIME) != 0) {
      if ((ea.rk & EK_SLAB) != 0) {   // split-K partials of a layout without a K_SLAB instantiation
        store_slab();
        return;
      }
    }
    // resources (offsets below are relative to the batch-(z1, z2) origin folded into the base pointer)
    const int64_t oc = (int64_t)z1 * e.cbs1 + (int64_t)z2 * e.cbs2;
    const int64_t oa = (int64_t)z1 * e.abs1 + (int64_t)z2 * e.abs2;
    const int64_t orr = (int64_t)z1 * e.rbs1 + (int64_t)z2 * e.rbs2;
    const uint64_t ext_c = (uint64_t)((int64_t)(M - 1) * e.ldc + N);
    // EK_RUNTIME: the kind's bits are the launch's (ea.rk) — uniform runtime branches, same structure
    const uint32_t K = (EK & EK_RUNTIME) != 0 ? ea.rk : EK;
    rsrc16_t rC = mkres(nullptr, 0), rC16 = rC, rP32 = rC, rP16 = rC, rA = rC, rR = rC;
    if ((K & (EK_C32 | EK_BETA)) != 0) rC = mkres(e.C + oc, ext_c * 4);
    if ((K & EK_C16) != 0) rC16 = mkres(e.C16 + oc, ext_c * 2);
    rsrc16_t rC16b = rC;
    if ((K & EK_C16B) != 0) rC16b = mkres(e.C16b + oc, ext_c * 2);
    if ((K & EK_PRE32) != 0) rP32 = mkres(e.pre_out + oc, ext_c * 4);
    if ((K & EK_PRE16) != 0) rP16 = mkres(e.pre16 + oc, ext_c * 2);
    if ((K & EK_ABWD) != 0) {
      const uint64_t ext_a = (uint64_t)((int64_t)(M - 1) * e.ldaux + N);
      if ((K & EK_AUX16) != 0) rA = mkres(e.aux16 + oa, ext_a * 2);
      else rA = mkres(e.aux + oa, ext_a * 4);
    }
    if ((K & EK_RES) != 0) rR = mkres(e.residual + orr, (uint64_t)((int64_t)(M - 1) * e.ldr + N) * 4);
    // column-constant operands: the bias of this lane's four columns, per column tile
    float4 bias4[NJT];
    if ((K & EK_BIAS) != 0) {
      const float* bp = e.bias + (int64_t)z1 * e.biasbs1;
#pragma unroll
      for (int j = 0; j < NJT; ++j) {
        const int n = ncol0 + 16 * j + cq;
        bias4[j] = n < N ? *reinterpret_cast<const float4*>(bp + n) : make_float4(0.f, 0.f, 0.f, 0.f);
      }
    }
    // fused column sums (EK_CSUM): per 32-row band (two row tiles) -> partial row (mrow0 + 32 b) / 32; every
    // wave row block (64 / 96 / 128 rows) starts on a band, so each band has exactly one writer
    auto colsum_band = [&](float4 (&cs)[NJT], int b) __attribute__((always_inline)) {
      const int nprow = (M + 31) / 32, prow = mrow0 / 32 + b;
#pragma unroll
      for (int j = 0; j < NJT; ++j) {
#pragma unroll
        for (int o = 1; o < 16; o <<= 1) {
          cs[j].x += __shfl_xor(cs[j].x, o, 64); cs[j].y += __shfl_xor(cs[j].y, o, 64);
          cs[j].z += __shfl_xor(cs[j].z, o, 64); cs[j].w += __shfl_xor(cs[j].w, o, 64);
        }
        const int n = ncol0 + 16 * j + cq;
        if (rl == 0 && n < N && prow < nprow) *reinterpret_cast<float4*>(e.colsum_part + (int64_t)prow * N + n) = cs[j];
        cs[j] = make_float4(0.f, 0.f, 0.f, 0.f);
      }
    };
    const float alpha = e.alpha, beta = e.beta;
    const uint64_t sd = b2p_seed_eff(e.drop_seed, ea.epoch);
    const int act = e.act, act_bwd = e.act_bwd;
    // 16-B form of the 16-bit images (W; ea.wide16, decided per launch on the host). The packed values of two
    // adjacent column tiles j, j+1 trade 16-lane groups (v_permlane16_swap: groups 1 and 3 of tile j's
    // register with groups 0 and 2 of tile j+1's), after which lane group g holds 8 consecutive columns of
    // its row, 16 (j + (g & 1)) + 8 (g >> 1) .. + 7: one store instruction covers 16 rows x 64 contiguous
    // bytes (the 8-B form: 16 rows x 32 B), half the store instructions for the same bytes. Values, and the
    // order of the arithmetic on them, are those of the 8-B form. (aux16 read the same way, 16 B per lane and
    // swapped back, measured no different from the 8-B loads: the backward kinds' tail is the GELU' arithmetic,
    // profiles/r07a_epilogue_attribution.txt.)
    const int cw = 16 * ((lane >> 4) & 1) + 8 * (lane >> 5);
    auto swap2 = [](uint2& a, uint2& b) __attribute__((always_inline)) {
      const auto x = __builtin_amdgcn_permlane16_swap(a.x, b.x, false, false);
      const auto y = __builtin_amdgcn_permlane16_swap(a.y, b.y, false, false);
      a = make_uint2(x[0], y[0]);
      b = make_uint2(x[1], y[1]);
    };
    auto body = [&](auto wide) __attribute__((always_inline)) {
      constexpr bool W = decltype(wide)::value;
      float4 cs[NJT] = {};
      // per-element operands of one row tile (loaded one row tile ahead of its use)
      float4 Lc[NJT], Lr[NJT], La[NJT];
      auto load_row = [&](int i, float4 (&lc)[NJT], float4 (&lr)[NJT], float4 (&la)[NJT]) __attribute__((always_inline)) {
        const int m = mrow0 + 16 * i + rl;
#pragma unroll
        for (int j = 0; j < NJT; ++j) {
          const int n = ncol0 + 16 * j + cq;
          const bool ok = m < M && n < N;
          if ((K & EK_BETA) != 0) lc[j] = bld16(rC, ok ? (uint32_t)(((int64_t)m * e.ldc + n) * 4) : OOB);
          if ((K & EK_RES) != 0) lr[j] = bld16(rR, ok ? (uint32_t)(((int64_t)m * e.ldr + n) * 4) : OOB);
          if ((K & EK_ABWD) != 0) {
            if ((K & EK_AUX16) != 0)
              la[j] = bf16x4_to_f4(bld8(rA, ok ? (uint32_t)(((int64_t)m * e.ldaux + n) * 2) : OOB));
            else
              la[j] = bld16(rA, ok ? (uint32_t)(((int64_t)m * e.ldaux + n) * 4) : OOB);
          }
        }
      };
      const bool LOADS = (K & (EK_BETA | EK_RES | EK_ABWD)) != 0;
      // a runtime-kind wave of 8 row tiles has no registers for the one-row-ahead loads (they spilled)
      constexpr bool AHEAD = !((EK & EK_RUNTIME) != 0 && MI > 4);
      if (LOADS && AHEAD) load_row(0, Lc, Lr, La);
#pragma unroll
      for (int i = 0; i < MI; ++i) {
        float4 Nc[NJT], Nr[NJT], Na[NJT];
        if (LOADS) {
          if (!AHEAD) load_row(i, Lc, Lr, La);
          else if (i + 1 < MI) load_row(i + 1, Nc, Nr, Na);
        }
        const int m = mrow0 + 16 * i + rl;
        const uint64_t drow = ((uint64_t)z * (uint64_t)M + (uint64_t)m) * (uint64_t)N;
        uint2 hP[NJT], hC[NJT], hB[NJT];   // W: the packed 16-bit images of a tile pair, until its second tile is done
#pragma unroll
        for (int j = 0; j < NJT; ++j) {
          const int n = ncol0 + 16 * j + cq;
          const bool ok = m < M && n < N;
          float v[4] = {alpha * acc[i][j][0], alpha * acc[i][j][1], alpha * acc[i][j][2], alpha * acc[i][j][3]};
          if ((K & EK_BETA) != 0) {
            v[0] += beta * Lc[j].x; v[1] += beta * Lc[j].y; v[2] += beta * Lc[j].z; v[3] += beta * Lc[j].w;
          }
          if ((K & EK_BIAS) != 0) {
            v[0] += bias4[j].x; v[1] += bias4[j].y; v[2] += bias4[j].z; v[3] += bias4[j].w;
          }
          const uint32_t o4 = ok ? (uint32_t)(((int64_t)m * e.ldc + n) * 4) : OOB;
          const uint32_t o2 = ok ? (uint32_t)(((int64_t)m * e.ldc + n) * 2) : OOB;
          if ((K & EK_PRE32) != 0) bst16(rP32, o4, make_float4(v[0], v[1], v[2], v[3]));
          if ((K & EK_PRE16) != 0) {
            const uint2 h = b2p_pack_bf16x4(make_float4(v[0], v[1], v[2], v[3]));
            if constexpr (W) hP[j] = h;
            else bst8(rP16, o2, h);
          }
          if ((K & EK_ACT) != 0) {
            if (act == B2P_ACT_GELU) {
              const b2p_f2 g0 = b2p_gelu2(b2p_f2{v[0], v[1]}), g1 = b2p_gelu2(b2p_f2{v[2], v[3]});
              v[0] = g0.x; v[1] = g0.y; v[2] = g1.x; v[3] = g1.y;
            } else {
#pragma unroll
              for (int q = 0; q < 4; ++q) v[q] = apply_act(v[q], act);
            }
          }
          if ((K & EK_DROP) != 0) {
            bool k[4];
            b2p_keep4(sd, drow + (uint64_t)n, ea.drop_thr, k);
#pragma unroll
            for (int q = 0; q < 4; ++q) v[q] = k[q] ? v[q] * ea.drop_scale : 0.0f;
          }
          if ((K & EK_ABWD) != 0) {
            if (act_bwd == B2P_ACT_GELU) {
              const b2p_f2 g0 = b2p_gelu_grad2(b2p_f2{La[j].x, La[j].y}), g1 = b2p_gelu_grad2(b2p_f2{La[j].z, La[j].w});
              v[0] *= g0.x; v[1] *= g0.y; v[2] *= g1.x; v[3] *= g1.y;
            } else {
              v[0] *= act_grad(La[j].x, act_bwd); v[1] *= act_grad(La[j].y, act_bwd);
              v[2] *= act_grad(La[j].z, act_bwd); v[3] *= act_grad(La[j].w, act_bwd);
            }
          }
          if ((K & EK_RES) != 0) {
            v[0] += Lr[j].x; v[1] += Lr[j].y; v[2] += Lr[j].z; v[3] += Lr[j].w;
          }
          const float4 f = make_float4(v[0], v[1], v[2], v[3]);
          if ((K & EK_C32) != 0) bst16(rC, o4, f);
          if ((K & EK_C16) != 0) {
            const uint2 h = (K & EK_C16H) != 0 ? b2p_pack_f16x4(f) : b2p_pack_bf16x4(f);
            if constexpr (W) hC[j] = h;
            else bst8(rC16, o2, h);
          }
          if ((K & EK_C16B) != 0) {
            const uint2 h = b2p_pack_bf16x4(f);
            if constexpr (W) hB[j] = h;
            else bst8(rC16b, o2, h);
          }
          if constexpr (W) {
            if (j & 1) {   // the pair (j - 1, j): 16 B per lane
              const int n8 = ncol0 + 16 * (j - 1) + cw;
              const uint32_t ow = (m < M && n8 < N) ? (uint32_t)(((int64_t)m * e.ldc + n8) * 2) : OOB;
              if ((K & EK_PRE16) != 0) {
                swap2(hP[j - 1], hP[j]);
                bst16u(rP16, ow, make_uint4(hP[j - 1].x, hP[j - 1].y, hP[j].x, hP[j].y));
              }
              if ((K & EK_C16) != 0) {
                swap2(hC[j - 1], hC[j]);
                bst16u(rC16, ow, make_uint4(hC[j - 1].x, hC[j - 1].y, hC[j].x, hC[j].y));
              }
              if ((K & EK_C16B) != 0) {
                swap2(hB[j - 1], hB[j]);
                bst16u(rC16b, ow, make_uint4(hB[j - 1].x, hB[j - 1].y, hB[j].x, hB[j].y));
              }
            }
          }
          if constexpr ((EK & EK_CSUM) != 0) {
            if (ok) { cs[j].x += f.x; cs[j].y += f.y; cs[j].z += f.z; cs[j].w += f.w; }
          }
        }
        if (LOADS && AHEAD) {
#pragma unroll
          for (int j = 0; j < NJT; ++j) { Lc[j] = Nc[j]; Lr[j] = Nr[j]; La[j] = Na[j]; }
        }
        if constexpr ((EK & EK_CSUM) != 0) {   // the host never hands column sums to EK_RUNTIME
          if (i & 1) colsum_band(cs, i >> 1);
        }
      }
    };
    // the runtime kind keeps the 8-B form: with both forms in it, it spilled (68-84 bytes of scratch per lane)
    constexpr bool WIDE_OK = NJT % 2 == 0 && (EK & EK_RUNTIME) == 0 && (EK & (EK_C16 | EK_C16B | EK_PRE16)) != 0;
    if constexpr (WIDE_OK) {
      if (ea.wide16) body(std::true_type{});
      else body(std::false_type{});
    } else {
      body(std::false_type{});
    }
  }
}

// Split-K fix-up inside the GEMM (ea.tile_ctr): every K-slice workgroup of a tile stores its fp32
// slab write-through (sc1), drains (every wave: vmcnt(0), then the workgroup's barrier) and counts
// itself in with one relaxed agent-scope vector atomic; the last one to arrive reads the tile's slabs
// with sc1 loads, sums them in slice order exactly as splitk_reduce4 does (bitwise the same C) and
// writes C (alpha / beta) and C16. (A __threadfence() release / acquire pair instead wrote back and
// invalidated the L2 per workgroup: base 15.4 -> 19.3 ms per step.)
// Replaces one reduce launch over the whole output per split-K GEMM (the weight gradients); the sums
// run in the tails of the K loops, the slabs still warm in L2 / MALL.
template <int NT>
__device__ __forceinline__ void splitk_fixup(const EpiArgs& ea, const b2p_gemm_desc& d, int z, int tile, int ks,
                                             int m0, int n0, int BM, int BN, char* smem) {
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // R1: every storing wave drains its sc1 slab stores
  __syncthreads();
  int* last = reinterpret_cast<int*>(smem);
  if (threadIdx.x == 0) {
    const uint32_t old = __hip_atomic_fetch_add(ea.tile_ctr + tile, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    *last = old == (uint32_t)(ks - 1);
  }
  __syncthreads();
  if (!*last) return;
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");   // no instruction: keeps the loads below the count
  const int M = (int)d.M, N = (int)d.N;
  const b2p_epilogue& e = ea.e;
  const int64_t MN = (int64_t)M * N;
  const float* ws = d.workspace + (int64_t)z * ks * MN;
  const rsrc16_t rws = mkres(ws, (uint64_t)ks * MN * 4);
  const int z1 = z / d.nz2, z2 = z - z1 * d.nz2;
  const int64_t cb = (int64_t)z1 * e.cbs1 + (int64_t)z2 * e.cbs2;
  const int mrows = (M - m0 < BM ? M - m0 : BM), ncols = (N - n0 < BN ? N - n0 : BN);
  const int c4n = (ncols + 3) >> 2;
  for (int i = threadIdx.x; i < mrows * c4n; i += NT) {
    const int r = i / c4n, c = 4 * (i - r * c4n);
    const int64_t off = (int64_t)(m0 + r) * N + n0 + c;
    float4 sacc = bld16_sc1(rws, (uint32_t)(off * 4));
    for (int q = 1; q < ks; ++q) {
      const float4 v = bld16_sc1(rws, (uint32_t)((q * MN + off) * 4));
      sacc.x += v.x; sacc.y += v.y; sacc.z += v.z; sacc.w += v.w;
    }
    const int64_t coff = cb + (int64_t)(m0 + r) * e.ldc + n0 + c;
    float4 v = make_float4(e.alpha * sacc.x, e.alpha * sacc.y, e.alpha * sacc.z, e.alpha * sacc.w);
    if (e.beta != 0.f) {
      const float4 cv = *reinterpret_cast<const float4*>(e.C + coff);
      v.x += e.beta * cv.x; v.y += e.beta * cv.y; v.z += e.beta * cv.z; v.w += e.beta * cv.w;
    }
    if (e.C) *reinterpret_cast<float4*>(e.C + coff) = v;
    if (e.C16) *reinterpret_cast<uint2*>(e.C16 + coff) = b2p_pack16x4(v, e.flags & B2P_EPI_C16_FP16);
  }
}

// output tile of linear tile index t: row-major (grp = 0), or grouped (grp > 0): column sweeps over
// bands of grp row tiles, so the workgroups resident on one XCD at a time share a few A row panels
// and a few B column panels in that XCD's L2 instead of cycling through all of B
// grp < 0: column bands of G = (tiles_n <= 8 ? tiles_n : ceil(tiles_n / 8)) output columns, row-major
// inside a band: the workgroups of one XCD (a contiguous range of this order, see the remap) then hold
// a G-column slice of B in their L2 while every A row panel they fetch feeds G tiles running side by side
__device__ __forceinline__ void tile_of(int t, int tiles_m, int tiles_n, int grp, int& tm, int& tn) {
  if (grp < 0) {
    const int G = tiles_n <= 8 ? tiles_n : (tiles_n + 7) / 8;
    const int per = G * tiles_m;
    const int band = t / per, r = t - band * per;
    const int gs = tiles_n - band * G < G ? tiles_n - band * G : G;
    tm = r / gs;
    tn = band * G + (r - tm * gs);
  } else if (grp > 0) {
    const int per = grp * tiles_n;
    const int g = t / per, first = g * grp;
    const int gs = tiles_m - first < grp ? tiles_m - first : grp;
    const int r = t - g * per;
    tn = r / gs;
    tm = first + (r - tn * gs);
  } else {
    tm = t / tiles_n;
    tn = t - tm * tiles_n;
  }
}

// Tile configurations: BM x BN output tile, WGM x WGN waves of WTM x 64 each ((WTM/16) x 4 MFMA tiles),
// KT-deep k-tiles, S LDS stages (S-1 tiles in flight behind counted vmcnt waits + raw barriers).
template <int BM_, int BN_, int KT_, int S_, int WTM_ = 64>
struct Cfg {
  static constexpr int BM = BM_, BN = BN_, KT = KT_, S = S_, WTM = WTM_, MI = WTM_ / 16;
  static constexpr int WGM = BM / WTM, WGN = BN / 64, NW = WGM * WGN, NT = NW * 64;
  static constexpr int STAGE = (BM + BN) * KT * 2;
  static constexpr int LDS = S * STAGE;                         // the epilogue works from registers
  static constexpr int OCC = LDS > 80 * 1024 ? 1 : 2;           // workgroups per CU
};
using CfgSmall = Cfg<128, 128, 32, 3>;   // 4 waves, 3 workgroups/CU by LDS (48 KB) and VGPRs (143)
// Measured and removed (DESIGN.md "rejected"): 128 x 128 x 64 two-stage tiles (Cfg<128, 128, 64, 2>: half
// the barriers per K, no gain inside the step), 256 x 128 tiles of 4 waves with 128 x 64 wave tiles
// (Cfg<256, 128, 32, 3, 128>: a quarter less operand traffic per FLOP, 72 KB of LDS, never the default),
// 128 x 64 tiles for N <= 1024 grids (59.3 -> 57.1 steps/s), 4-stage 128 x 128 x 32 (-10 % at K = 768),
// 256 x 128 x 64 eight-wave tiles (lock-stepped waves idle the MFMA pipe at every barrier).

// H16: the operands are fp16 (Operand.dtype 2, precision 2) and feed v_mfma_f32_16x16x32_f16; the
// data movement is the same 16-bit copy either way
template <class CF, bool AK, bool BK, bool ACONV, bool H16, uint32_t EK>
__global__ void __launch_bounds__(CF::NT, CF::OCC) gemm16_kernel(const b2p_gemm_desc d, const EpiArgs ea, int tiles_m,
                                                                int tiles_n, int grp) {
  constexpr int BM = CF::BM, BN = CF::BN, KT = CF::KT, S = CF::S, NT = CF::NT;
  constexpr int A_BYTES = BM * KT * 2;
  constexpr int STAGE_BYTES = CF::STAGE;
  using SA = Src<BM, KT, AK, ACONV, CF::NW>;
  using SB = Src<BN, KT, BK, false, CF::NW>;
  constexpr int PT = SA::NI + SB::NI;                          // glds per wave per tile (A + B)
  __shared__ __attribute__((aligned(1024))) char smem[CF::LDS];

  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm = wave / CF::WGN, wn = wave % CF::WGN;

  // XCD-aware remap (bijective): blocks with equal blockIdx.x % 8 share an XCD and its L2, so
  // give each such group a contiguous range of tiles (neighbouring tiles share A rows).
  const int nwg = gridDim.x;
  const int orig = blockIdx.x;
  const int xcd = orig & 7, q8 = nwg >> 3, r8 = nwg & 7;
  const int wgid = (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + (orig >> 3);
  const int tiles = tiles_m * tiles_n;
  const int zz = wgid / tiles;
  const int t = wgid - zz * tiles;
  int tm, tn;
  tile_of(t, tiles_m, tiles_n, grp, tm, tn);

  const int ks = d.ksplit > 1 ? d.ksplit : 1;
  const int z = zz / ks, ksl = zz - z * ks;
  const int z1 = z / d.nz2, z2 = z - z1 * d.nz2;
  const int m0 = tm * BM, n0 = tn * BN;
  const int M = (int)d.M, N = (int)d.N;
  const int kchunk = ks > 1 ? (int)d.kchunk : (int)d.K;
  const int kbeg = ksl * kchunk;
  const int K = ((int)d.K < kbeg + kchunk) ? (int)d.K : kbeg + kchunk;
  const int nk = (K > kbeg && !b2p_gated_off(gemm_gate<EK>(ea, z1))) ? (K - kbeg + KT - 1) / KT : 0;

  SA sa;
  SB sb;
  sa.init(d.A, z1, z2, wave, lane, m0, M, kbeg);
  sb.init(d.B, z1, z2, wave, lane, n0, N, kbeg);

  constexpr int MI = CF::MI;
  f32x4 acc[MI][4];
#pragma unroll
  for (int i = 0; i < MI; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  // prologue: S-1 tiles in flight
#pragma unroll
  for (int s = 0; s < S - 1; ++s) {
    if (s < nk) {
      sa.issue(smem + s * STAGE_BYTES, wave, kbeg + s * KT, K);
      sb.issue(smem + s * STAGE_BYTES + A_BYTES, wave, kbeg + s * KT, K);
    }
  }
  int cur = 0;              // stage of tile kt
  int nxt = S - 1;          // stage receiving tile kt + S - 1
  for (int kt = 0; kt < nk; ++kt) {
    // this wave's share of tile kt has landed (later tiles may stay in flight) ...
    if (kt + S - 2 < nk) wait_vm<(S - 2) * PT>();
    else wait_vm<0>();
    // ... and everyone's has; every wave is also done reading stage kt-1 (= nxt)
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    if (kt + S - 1 < nk) {
      char* img = smem + nxt * STAGE_BYTES;
      sa.issue(img, wave, kbeg + (kt + S - 1) * KT, K);
      sb.issue(img + A_BYTES, wave, kbeg + (kt + S - 1) * KT, K);
    }
    const char* As = smem + cur * STAGE_BYTES;
    const char* Bs = As + A_BYTES;
#pragma unroll
    for (int kk = 0; kk < KT / 32; ++kk) {
      bf16x8 bfr[4];
#pragma unroll
      for (int j = 0; j < 4; ++j)
        bfr[j] = BK ? frag_k<KT>(Bs, wn * 64 + j * 16, kk, lane) : frag_t<BN>(Bs, wn * 64 + j * 16, kk, lane);
      // A fragments in groups of 4 rows of MFMA tiles: at most 8 fragments live beside the
      // (MI x 4) accumulators (the 128-row wave tile would otherwise exceed 256 registers)
#pragma unroll
      for (int i0 = 0; i0 < MI; i0 += 4) {
        bf16x8 af[4];
#pragma unroll
        for (int i = 0; i < 4; ++i)
          af[i] = AK ? frag_k<KT>(As, wm * CF::WTM + (i0 + i) * 16, kk, lane)
                     : frag_t<BM>(As, wm * CF::WTM + (i0 + i) * 16, kk, lane);
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int j = 0; j < 4; ++j)
            // operand roles swapped: the accumulator tile is the transposed output block (register epilogue)
            if constexpr (H16)
              acc[i0 + i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(
                  __builtin_bit_cast(f16x8g, bfr[j]), __builtin_bit_cast(f16x8g, af[i]), acc[i0 + i][j], 0, 0, 0);
            else
              acc[i0 + i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bfr[j], af[i], acc[i0 + i][j], 0, 0, 0);
      }
    }
    cur = cur + 1 == S ? 0 : cur + 1;
    nxt = nxt + 1 == S ? 0 : nxt + 1;
  }

  float* slab = ks > 1 ? d.workspace + ((int64_t)z * ks + ksl) * (int64_t)M * N : nullptr;
  static_assert(CF::LDS >= gen_lds_bytes(CF::NW), "GENERIC epilogue staging exceeds the LDS");
  reg_epilogue<EK, MI>(ea, d, acc, z, z1, z2, m0 + wm * CF::WTM, n0 + wn * 64, lane, slab, smem);
  if (slab && ea.tile_ctr) splitk_fixup<CF::NT>(ea, d, z, z * tiles + t, ks, m0, n0, BM, BN, smem);
}

// ------------------------------------------------------------------------------------------------
// 256 x 256 x 64 ping-pong kernel: 8 waves in two groups of 4 (group g owns output rows
// 128g .. 128g+127, wave wc of the group columns 64wc .. 64wc+63: a 128 x 64 sub-tile, 8 x 4 MFMA
// tiles). Every K-tile runs in 4 phases, one output quadrant (64 x 32, K 64 = 16 MFMAs) each:
//     ds_read this quadrant's fragments, [issue LDS-DMA of the next K-tile], lgkmcnt(0), barrier,
//     16 MFMAs, barrier.
// Group 1 starts one barrier later than group 0, so on every SIMD (one wave of each group) one wave
// feeds the matrix pipe while its partner reads fragments and issues DMA. Two LDS buffers: tile
// kt+1 is DMA'd into the idle buffer in phases 0 (A) and 1 (B) of tile kt and waited for
// (vmcnt(0)) in phase 3 before that phase's first barrier, so every reader of tile kt+1 passes a
// barrier after every issuer's wait. Every fragment read is retired (lgkmcnt(0)) before the
// phase's first barrier, so the buffer a DMA overwrites has no read in flight (WAR).
#ifdef B2P_PP_STAMPS   // diagnostic build only (tools/pp_probe.hip): per-workgroup clock stamps
__device__ unsigned long long g_pp_stamps[8 * 8192];
__device__ int g_pp_diag;   // bits: 1 = no K-loop DMA, 2 = no MFMA, 4 = no fragment reads (timing only)
#define PP_DIAG g_pp_diag
#define PP_STAMP(k)                                                                          \
  do {                                                                                       \
    if (tid == 0 && blockIdx.x < 8192) {                                                     \
      g_pp_stamps[(size_t)blockIdx.x * 8 + (k)] = __builtin_amdgcn_s_memtime();              \
      g_pp_stamps[(size_t)blockIdx.x * 8 + 4 + (k)] = __builtin_amdgcn_s_memrealtime();      \
    }                                                                                        \
  } while (0)
#else
#define PP_STAMP(k)
#define PP_DIAG 0
#endif

constexpr int PP_NT = 512;
constexpr int PP_KT = 64;
constexpr int PP_BBYTES = 256 * PP_KT * 2;              // 32 KB: the B image of one buffer
// PBM = 256 (two 128-row wave groups) or 192 (two 96-row groups: 42 x 12 = 504 tiles at 7968 x 3072,
// two full rounds of the 256 CUs instead of 384 = 1.5); A k-contiguous only for 192 (the m-contiguous
// image needs 128-column chunks per k-row)
template <int PBM> constexpr int pp_abytes() { return PBM * PP_KT * 2; }
template <int PBM> constexpr int pp_stage() { return pp_abytes<PBM>() + PP_BBYTES; }
template <int PBM> constexpr int pp_lds() { return 2 * pp_stage<PBM>(); }

__device__ __forceinline__ void pp_barrier() {
  __builtin_amdgcn_sched_barrier(0);
  asm volatile("s_barrier" ::: "memory");
  __builtin_amdgcn_sched_barrier(0);
}
__device__ __forceinline__ void pp_lgkm0() {
  __builtin_amdgcn_sched_barrier(0);
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  __builtin_amdgcn_sched_barrier(0);
}

template <int PBM, bool AK, bool BK, bool H16, uint32_t EK>
__global__ void __launch_bounds__(PP_NT, 1) gemm16_pp_kernel(const b2p_gemm_desc d, const EpiArgs ea, int tiles_m,
                                                            int tiles_n, int grp) {
  static_assert(PBM == 256 || (PBM == 192 && AK), "ping-pong tile rows: 256, or 192 with a k-contiguous A");
  constexpr int MI = PBM / 32;           // 16-row MFMA tiles per wave (two phase halves of MI / 2)
  constexpr int HM = MI / 2;
  constexpr int PP_ABYTES = pp_abytes<PBM>(), PP_STAGE = pp_stage<PBM>();
  // quarter-scheduled DMA (256-row k-contiguous operands): see the K loop below
  constexpr bool QS = PBM == 256 && AK && BK;
  // phase 3 reuses phase 0's B fragments (16 VGPRs) instead of reading them again; the runtime-kind
  // epilogue has no registers left for them
  constexpr bool KEEPB = EK != EK_RUNTIME;
  using SA = SrcB<PBM, PP_KT, AK, 8, QS ? 1 : 0>;
  using SB = SrcB<256, PP_KT, BK, 8, QS ? 2 : 0>;
  __shared__ __attribute__((aligned(1024))) char smem[pp_lds<PBM>()];

  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int g = wave >> 2, wc = wave & 3;
  PP_STAMP(0);

  const int nwg = gridDim.x;
  const int orig = blockIdx.x;
  const int xcd = orig & 7, q8 = nwg >> 3, r8 = nwg & 7;
  const int wgid = (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + (orig >> 3);
  const int tiles = tiles_m * tiles_n;
  const int zz = wgid / tiles;
  const int t = wgid - zz * tiles;
  int tm, tn;
  tile_of(t, tiles_m, tiles_n, grp, tm, tn);

  const int ks = d.ksplit > 1 ? d.ksplit : 1;
  const int z = zz / ks, ksl = zz - z * ks;
  const int z1 = z / d.nz2, z2 = z - z1 * d.nz2;
  const int m0 = tm * PBM, n0 = tn * 256;
  const int M = (int)d.M, N = (int)d.N;
  const int kchunk = ks > 1 ? (int)d.kchunk : (int)d.K;
  const int kbeg = ksl * kchunk;
  const int K = ((int)d.K < kbeg + kchunk) ? (int)d.K : kbeg + kchunk;
  const int nk = (K > kbeg && !b2p_gated_off(gemm_gate<EK>(ea, z1))) ? (K - kbeg + PP_KT - 1) / PP_KT : 0;

  SA sa;
  SB sb;
  sa.init(d.A, z1, z2, wave, lane, m0, M, (int)d.K, kbeg);
  sb.init(d.B, z1, z2, wave, lane, n0, N, (int)d.K, kbeg);

  f32x4 acc[MI][4];
#pragma unroll
  for (int i = 0; i < MI; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  if (nk > 0) {
    if constexpr (QS) {   // quarters in the order the loop waits for them; A q0 and B q0 first
      sa.template issue_q<0>(smem, wave, lane, kbeg, K);
      sb.template issue_q<0>(smem + PP_ABYTES, wave, lane, kbeg, K);
      sb.template issue_q<1>(smem + PP_ABYTES, wave, lane, kbeg, K);
      sa.template issue_q<1>(smem, wave, lane, kbeg, K);
      wait_vm<4>();
    } else {
      sa.issue(smem, wave, lane, kbeg, K);
      sb.issue(smem + PP_ABYTES, wave, lane, kbeg, K);
      wait_vm<0>();
    }
  }
  pp_barrier();
  if (g == 1) pp_barrier();   // the stagger
  PP_STAMP(1);

  bf16x8 a[HM][2], b[2][2], b0k[2][2];
  const int arow = g * (PBM / 2), bcol = wc * 64;
  const int diag = PP_DIAG;
  auto readA = [&](const char* As, int mi) {
    if (diag & 4) return;
#pragma unroll
    for (int i = 0; i < HM; ++i)
#pragma unroll
      for (int kk = 0; kk < 2; ++kk)
        a[i][kk] = AK ? frag_k<PP_KT>(As, arow + mi * (PBM / 4) + i * 16, kk, lane)
                      : frag_t<PBM>(As, arow + mi * (PBM / 4) + i * 16, kk, lane);
  };
  auto readB = [&](const char* Bs, int nj) {
    if (diag & 4) return;
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int kk = 0; kk < 2; ++kk)
        b[j][kk] = BK ? frag_k<PP_KT>(Bs, bcol + nj * 32 + j * 16, kk, lane)
                      : frag_t<256>(Bs, bcol + nj * 32 + j * 16, kk, lane);
  };
  auto mfma_b = [&](int mi, int nj, const bf16x8 (&bb)[2][2]) {
    if (diag & 2) return;
    __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int i = 0; i < HM; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int kk = 0; kk < 2; ++kk)
          if constexpr (H16)   // operand roles swapped (register epilogue)
            acc[mi * HM + i][nj * 2 + j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(
                __builtin_bit_cast(f16x8g, bb[j][kk]), __builtin_bit_cast(f16x8g, a[i][kk]), acc[mi * HM + i][nj * 2 + j],
                0, 0, 0);
          else
            acc[mi * HM + i][nj * 2 + j] =
                __builtin_amdgcn_mfma_f32_16x16x32_bf16(bb[j][kk], a[i][kk], acc[mi * HM + i][nj * 2 + j], 0, 0, 0);
    __builtin_amdgcn_s_setprio(0);
  };
  auto mfma = [&](int mi, int nj) { mfma_b(mi, nj, b); };

  // Quarter-scheduled K loop (QS). The images of K-tile kt+1 load in four quarters, one per phase of kt,
  // each 2 DMAs per wave: A q0 (rows of the mi = 0 halves) in phase 0, B q0 (nj = 0 columns) in phase 1,
  // B q1 in phase 2, A q1 in phase 3; phase 3 computes its quadrant from the B nj = 0 fragments phase 0
  // read (kept in registers), so the last LDS read of a K-tile is phase 2's. Every quarter is waited for
  // (counted vmcnt, younger quarters left in flight) in the read section of the phase before its first
  // reader: A q0 + B q0 in phase 3 of kt, B q1 in phase 0 and A q1 in phase 1 of kt+1. The 2-buffer kernel
  // issued 4 DMAs per wave in each of phases 0 and 1 and waited for all of them in phase 3 (its K loop
  // measured as long as its DMA alone, DESIGN.md section 5). WAR: a quarter of kt+1 overwrites the same
  // quarter of kt-1, whose last read (phase 2 of kt-1 at the latest) every wave retired before a barrier
  // both groups passed before phase 0 of kt.
  if constexpr (QS) {
    for (int kt = 0; kt < nk; ++kt) {
      const char* As = smem + (kt & 1) * PP_STAGE;
      const char* Bs = As + PP_ABYTES;
      char* nx = smem + ((kt + 1) & 1) * PP_STAGE;
      const bool n1 = kt + 1 < nk && !(diag & 1);
      const int knext = kbeg + (kt + 1) * PP_KT;
      // phase 0: quadrant (0, 0); DMA A q0 of kt+1; B q1 of kt must land
      readA(As, 0);
      readB(Bs, 0);
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) b0k[j][kk] = b[j][kk];
      if (n1) {
        sa.template issue_q<0>(nx, wave, lane, knext, K);
        wait_vm<4>();
      } else {
        wait_vm<2>();
      }
      pp_lgkm0();
      pp_barrier();
      mfma(0, 0);
      pp_barrier();
      // phase 1: quadrant (0, 1); DMA B q0 of kt+1; A q1 of kt must land
      readB(Bs, 1);
      if (n1) {
        sb.template issue_q<0>(nx + PP_ABYTES, wave, lane, knext, K);
        wait_vm<4>();
      } else {
        wait_vm<0>();
      }
      pp_lgkm0();
      pp_barrier();
      mfma(0, 1);
      pp_barrier();
      // phase 2: quadrant (1, 1); DMA B q1 of kt+1
      readA(As, 1);
      if (n1) sb.template issue_q<1>(nx + PP_ABYTES, wave, lane, knext, K);
      pp_lgkm0();
      pp_barrier();
      mfma(1, 1);
      pp_barrier();
      // phase 3: quadrant (1, 0) from the kept B fragments; DMA A q1 of kt+1; A q0 + B q0 of kt+1 must land
      if (n1) {
        sa.template issue_q<1>(nx, wave, lane, knext, K);
        wait_vm<4>();
      }
      pp_lgkm0();
      pp_barrier();
      mfma_b(1, 0, b0k);
      pp_barrier();
    }
  } else
  for (int kt = 0; kt < nk; ++kt) {
    const char* As = smem + (kt & 1) * PP_STAGE;
    const char* Bs = As + PP_ABYTES;
    char* nx = smem + ((kt + 1) & 1) * PP_STAGE;
    const bool more = kt + 1 < nk;
    const int knext = kbeg + (kt + 1) * PP_KT;
    // phase 0: quadrant (0, 0); DMA A of tile kt+1; the B nj = 0 fragments stay in registers for phase 3
    readA(As, 0);
    readB(Bs, 0);
    if constexpr (KEEPB) {
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) b0k[j][kk] = b[j][kk];
    }
    if (more && !(diag & 1)) sa.issue(nx, wave, lane, knext, K);
    pp_lgkm0();
    pp_barrier();
    mfma(0, 0);
    pp_barrier();
    // phase 1: quadrant (0, 1); DMA B of tile kt+1
    readB(Bs, 1);
    if (more && !(diag & 1)) sb.issue(nx + PP_ABYTES, wave, lane, knext, K);
    pp_lgkm0();
    pp_barrier();
    mfma(0, 1);
    pp_barrier();
    // phase 2: quadrant (1, 1)
    readA(As, 1);
    pp_lgkm0();
    pp_barrier();
    mfma(1, 1);
    pp_barrier();
    // phase 3: quadrant (1, 0) from the kept B fragments (no LDS read: the m/n-contiguous layouts read every
    // fragment with two transpose reads); tile kt+1 must have landed before this phase's first barrier
    if constexpr (!KEEPB) readB(Bs, 0);
    wait_vm<0>();
    pp_lgkm0();
    pp_barrier();
    if constexpr (KEEPB) mfma_b(1, 0, b0k);
    else mfma(1, 0);
    pp_barrier();
  }
  if (g == 0) pp_barrier();   // equal barrier counts for both groups
  PP_STAMP(2);

  float* slab = ks > 1 ? d.workspace + ((int64_t)z * ks + ksl) * (int64_t)M * N : nullptr;
  static_assert(pp_lds<PBM>() >= gen_lds_bytes(PP_NT / 64), "GENERIC epilogue staging exceeds the LDS");
  reg_epilogue<EK, MI>(ea, d, acc, z, z1, z2, m0 + g * (PBM / 2), n0 + wc * 64, lane, slab, smem);
  if (slab && ea.tile_ctr) splitk_fixup<PP_NT>(ea, d, z, z * tiles + t, ks, m0, n0, PBM, 256, smem);
  PP_STAMP(3);
}

// ------------------------------------------------------------------------------------------------
// Narrow ping-pong kernel (round 6): PBM x 128 output tiles (PBM = 256 or 192), both operands
// k-contiguous, for the N <= 1024 encoder GEMMs (the residual-adding backward-data GEMMs, the FFN2 /
// out-projection forwards, dO): 192 x 128 tiles give 42 x 6 = 252 workgroups at N = 768 and 256 x 128 give
// 32 x 8 = 256 at N = 1024, one round of the 256 CUs, where 256-column tiles leave half the chip idle and
// the 128 x 128 kernel runs 1.5 rounds of 2-3 workgroups per CU. The ping-pong wave layout (8 waves, two
// groups of 4 staggered by one barrier; group g owns rows PBM/2 g .., wave wc columns 32 wc ..; a
// (PBM/2) x 32 wave tile) with two phases per 64-deep K-tile, one 64-row (48-row) half of the wave tile
// each (16 / 12 MFMAs): phase 0 reads the A half and both B fragments, phase 1 the other A half. The
// operand images (48 / 40 KB per K-tile) rotate through 3 LDS stages, so two K-tiles of DMA are in flight:
// K-tile kt+2's A is issued in phase 0 of kt and its B in phase 1, and phase 1 waits (counted vmcnt) for
// kt+1. WAR: stage (kt+2) % 3 held kt-1, whose last reads (phase 1 of kt-1) every wave retired before a
// barrier both groups passed before phase 0 of kt. RAW: every wave waits for its share of kt+1 before the
// barrier that precedes the first read of kt+1.
constexpr int PN_STAGES = 3;
template <int PBM> constexpr int pn_abytes() { return PBM * PP_KT * 2; }
constexpr int PN_BBYTES = 128 * PP_KT * 2;
template <int PBM> constexpr int pn_stage() { return pn_abytes<PBM>() + PN_BBYTES; }

template <int PBM, bool H16, uint32_t EK>
__global__ void __launch_bounds__(PP_NT, 1) gemm16_pn_kernel(const b2p_gemm_desc d, const EpiArgs ea, int tiles_m,
                                                            int tiles_n, int grp) {
  static_assert(PBM == 256 || PBM == 192, "narrow tile rows: 256 or 192");
  static_assert(EK != EK_GENERIC, "the narrow kernel has no LDS-staged epilogue");
  constexpr int MI = PBM / 32;   // 16-row MFMA tiles per wave
  constexpr int HM = MI / 2;
  constexpr int ABYTES = pn_abytes<PBM>(), STAGE = pn_stage<PBM>();
  using SA = SrcB<PBM, PP_KT, true, 8>;
  using SB = SrcB<128, PP_KT, true, 8>;
  constexpr int GAB = SA::NI + SB::NI;   // DMAs per wave per K-tile
  __shared__ __attribute__((aligned(1024))) char smem[PN_STAGES * STAGE];

  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int g = wave >> 2, wc = wave & 3;

  const int nwg = gridDim.x;
  const int orig = blockIdx.x;
  const int xcd = orig & 7, q8 = nwg >> 3, r8 = nwg & 7;
  const int wgid = (xcd < r8 ? xcd * (q8 + 1) : r8 * (q8 + 1) + (xcd - r8) * q8) + (orig >> 3);
  const int tiles = tiles_m * tiles_n;
  const int zz = wgid / tiles;
  const int t = wgid - zz * tiles;
  int tm, tn;
  tile_of(t, tiles_m, tiles_n, grp, tm, tn);

  const int ks = d.ksplit > 1 ? d.ksplit : 1;
  const int z = zz / ks, ksl = zz - z * ks;
  const int z1 = z / d.nz2, z2 = z - z1 * d.nz2;
  const int m0 = tm * PBM, n0 = tn * 128;
  const int M = (int)d.M, N = (int)d.N;
  const int kchunk = ks > 1 ? (int)d.kchunk : (int)d.K;
  const int kbeg = ksl * kchunk;
  const int K = ((int)d.K < kbeg + kchunk) ? (int)d.K : kbeg + kchunk;
  const int nk = (K > kbeg && !b2p_gated_off(gemm_gate<EK>(ea, z1))) ? (K - kbeg + PP_KT - 1) / PP_KT : 0;

  SA sa;
  SB sb;
  sa.init(d.A, z1, z2, wave, lane, m0, M, (int)d.K, kbeg);
  sb.init(d.B, z1, z2, wave, lane, n0, N, (int)d.K, kbeg);

  f32x4 acc[MI][2];
#pragma unroll
  for (int i = 0; i < MI; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  // prologue: K-tiles 0 and 1 in flight, 0 landed
#pragma unroll
  for (int s = 0; s < 2; ++s)
    if (s < nk) {
      sa.issue(smem + s * STAGE, wave, lane, kbeg + s * PP_KT, K);
      sb.issue(smem + s * STAGE + ABYTES, wave, lane, kbeg + s * PP_KT, K);
    }
  if (nk > 1) wait_vm<GAB>();
  else wait_vm<0>();
  pp_barrier();
  if (g == 1) pp_barrier();   // the stagger

  bf16x8 a[HM][2], b[2][2];
  const int arow = g * (PBM / 2), bcol = wc * 32;
  auto readA = [&](const char* As, int mi) {
#pragma unroll
    for (int i = 0; i < HM; ++i)
#pragma unroll
      for (int kk = 0; kk < 2; ++kk) a[i][kk] = frag_k<PP_KT>(As, arow + mi * (PBM / 4) + i * 16, kk, lane);
  };
  auto readB = [&](const char* Bs) {
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int kk = 0; kk < 2; ++kk) b[j][kk] = frag_k<PP_KT>(Bs, bcol + j * 16, kk, lane);
  };
  auto mfma = [&](int mi) {
    __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int i = 0; i < HM; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int kk = 0; kk < 2; ++kk)
          if constexpr (H16)   // operand roles swapped (register epilogue)
            acc[mi * HM + i][j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(
                __builtin_bit_cast(f16x8g, b[j][kk]), __builtin_bit_cast(f16x8g, a[i][kk]), acc[mi * HM + i][j], 0, 0, 0);
          else
            acc[mi * HM + i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(b[j][kk], a[i][kk], acc[mi * HM + i][j], 0, 0, 0);
    __builtin_amdgcn_s_setprio(0);
  };

  int cur = 0;   // stage of K-tile kt; kt+2 goes to the stage kt-1 used
  for (int kt = 0; kt < nk; ++kt) {
    const char* As = smem + cur * STAGE;
    const char* Bs = As + ABYTES;
    const int nst = cur == 0 ? PN_STAGES - 1 : cur - 1;
    char* nx = smem + nst * STAGE;
    const bool n2 = kt + 2 < nk;
    const int k2 = kbeg + (kt + 2) * PP_KT;
    // phase 0: the first A half with both B fragments; DMA A of kt+2
    readA(As, 0);
    readB(Bs);
    if (n2) sa.issue(nx, wave, lane, k2, K);
    pp_lgkm0();
    pp_barrier();
    mfma(0);
    pp_barrier();
    // phase 1: the second A half; DMA B of kt+2; K-tile kt+1 must have landed
    readA(As, 1);
    if (n2) {
      sb.issue(nx + ABYTES, wave, lane, k2, K);
      __builtin_amdgcn_sched_barrier(0);
      wait_vm<GAB>();
    } else {
      __builtin_amdgcn_sched_barrier(0);
      wait_vm<0>();
    }
    pp_lgkm0();
    pp_barrier();
    mfma(1);
    pp_barrier();
    cur = cur == PN_STAGES - 1 ? 0 : cur + 1;
  }
  if (g == 0) pp_barrier();   // equal barrier counts for both groups

  float* slab = ks > 1 ? d.workspace + ((int64_t)z * ks + ksl) * (int64_t)M * N : nullptr;
  reg_epilogue<EK, MI, 2>(ea, d, acc, z, z1, z2, m0 + g * (PBM / 2), n0 + wc * 32, lane, slab, smem);
  if (slab && ea.tile_ctr) splitk_fixup<PP_NT>(ea, d, z, z * tiles + t, ks, m0, n0, PBM, 128, smem);
}

// ------------------------------------------------------------------------------------------------
// epilogue kinds with instantiations (everything else runs EK_GENERIC)
constexpr uint32_t K_F = EK_C32, K_FB = EK_C32 | EK_BETA, K_H = EK_C16, K_HH = EK_C16 | EK_C16H,
                   K_BH = EK_BIAS | EK_C16, K_BHH = EK_BIAS | EK_C16 | EK_C16H, K_BF = EK_BIAS | EK_C32,
                   K_RF = EK_RES | EK_C32, K_BDRF = EK_BIAS | EK_DROP | EK_RES | EK_C32,
                   K_DRF = EK_DROP | EK_RES | EK_C32,
                   K_BADH = EK_BIAS | EK_PRE16 | EK_ACT | EK_DROP | EK_C16,
                   K_BPADHH = EK_BIAS | EK_PRE32 | EK_ACT | EK_DROP | EK_C16 | EK_C16H,
                   K_BADHHB = EK_BIAS | EK_PRE16 | EK_ACT | EK_DROP | EK_C16 | EK_C16H | EK_C16B,
                   K_BPADHHB = K_BPADHH | EK_C16B,
                   K_GDH16CS = EK_DROP | EK_ABWD | EK_AUX16 | EK_C16 | EK_CSUM,
                   K_GDH16 = EK_DROP | EK_ABWD | EK_AUX16 | EK_C16,
                   K_GDH32CS = EK_DROP | EK_ABWD | EK_C16 | EK_CSUM, K_SLAB = EK_SLAB;
// bf16 operands, A and B k-contiguous (forward / backward-data GEMMs)
#define B2P_KINDS_NT_BF16(X) X(K_F) X(K_FB) X(K_H) X(K_BH) X(K_BF) X(K_RF) X(K_BDRF) X(K_DRF) X(K_BADH) \
  X(K_GDH16CS) X(K_GDH16) X(K_GDH32CS) X(K_SLAB)
// fp16 operands (forward_f16), A and B k-contiguous
#define B2P_KINDS_NT_F16(X) X(K_F) X(K_BF) X(K_BH) X(K_BHH) X(K_HH) X(K_RF) X(K_BDRF) X(K_DRF) X(K_BPADHH) X(K_BADHHB) \
  X(K_BPADHHB) X(K_SLAB)
// other layouts (weight gradients: A and B m/n-contiguous; backward-data with a [K][N] B)
#define B2P_KINDS_OTHER(X) X(K_F) X(K_FB) X(K_SLAB)

template <class CF, bool AK, bool BK, bool ACONV, bool H16, uint32_t EK>
void launch_small(const b2p_gemm_desc& d, const EpiArgs& ea, hipStream_t st, unsigned nwg, int tm, int tn, int grp) {
  hipLaunchKernelGGL((gemm16_kernel<CF, AK, BK, ACONV, H16, EK>), dim3(nwg), dim3(CF::NT), 0, st, d, ea, tm, tn, grp);
}
template <bool AK, bool BK, bool H16, uint32_t EK>
void launch_pp(const b2p_gemm_desc& d, const EpiArgs& ea, hipStream_t st, unsigned nwg, int tm, int tn, int grp) {
  hipLaunchKernelGGL((gemm16_pp_kernel<256, AK, BK, H16, EK>), dim3(nwg), dim3(PP_NT), 0, st, d, ea, tm, tn, grp);
}
template <int PBM, bool H16, uint32_t EK>
void launch_pn(const b2p_gemm_desc& d, const EpiArgs& ea, hipStream_t st, unsigned nwg, int tm, int tn, int grp) {
  if constexpr (EK == EK_GENERIC) {
    b2p_set_error("gemm16: the narrow kernel has no GENERIC epilogue");
  } else {
    hipLaunchKernelGGL((gemm16_pn_kernel<PBM, H16, EK>), dim3(nwg), dim3(PP_NT), 0, st, d, ea, tm, tn, grp);
  }
}
template <bool BK, bool H16, uint32_t EK>
void launch_pp192(const b2p_gemm_desc& d, const EpiArgs& ea, hipStream_t st, unsigned nwg, int tm, int tn, int grp) {
  hipLaunchKernelGGL((gemm16_pp_kernel<192, true, BK, H16, EK>), dim3(nwg), dim3(PP_NT), 0, st, d, ea, tm, tn, grp);
}

}  // namespace

// kernel families of one instantiation unit: 128 x 128 (CfgSmall), 256 x 256 ping-pong, 192 x 256
// ping-pong (k-contiguous A), 256 x 128 / 192 x 128 narrow ping-pong (both operands k-contiguous)
enum { G16_SMALL, G16_PP, G16_PP192, G16_PN256, G16_PN192 };
int gemm16_run_nt_bf16(const b2p_gemm_desc& d, hipStream_t st, int fam, uint32_t ek, unsigned nwg, int tm, int tn, int grp,
                       uint32_t* ctr);
int gemm16_run_nt_f16(const b2p_gemm_desc& d, hipStream_t st, int fam, uint32_t ek, unsigned nwg, int tm, int tn, int grp,
                      uint32_t* ctr);
int gemm16_run_other(const b2p_gemm_desc& d, hipStream_t st, int fam, uint32_t ek, unsigned nwg, int tm, int tn, int grp,
                     uint32_t* ctr);
