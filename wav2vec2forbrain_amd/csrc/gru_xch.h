// State exchange of the multi-CU persistent GRU recurrences (csrc/grumc.hip: 16-bit operands; csrc/gru32.hip:
// exact fp32): tagged 8-byte granules written by one vector atomic store and polled with a bounded spin,
// the placement of a recurrence's member workgroups, the one-XCD check that picks the store flavour, the
// kernel that zeroes a workspace before a launch, the workspace's carve-up and the entry points' shared
// argument checks. One copy of the bounded-spin path for both files.
#pragma once
#include "common.h"

namespace {
constexpr int XCH_NTH = 256;        // threads of a member workgroup (the sweep's lane stride)
constexpr unsigned SPIN_MAX = 1u << 22;
constexpr int IDS_PER_GROUP = 16;   // members' XCC ids (P <= 16; gru32.hip at H = 1024, P = 32, strides 32 of its own)

typedef __attribute__((address_space(1))) unsigned long long gu64;

// Granule stores: sc1 (write-through to memory: visible to any XCD) or, when every member of the
// recurrence runs on this XCD (checked at launch, see same_xcd), a workgroup-scope store (sc0: the
// line stays in the XCD's L2, where the other members' sc1 loads read it, ~2x closer than memory).
__device__ __forceinline__ void store_granule(unsigned long long* p, unsigned long long x, bool local) {
  if (local)
    __hip_atomic_store((gu64*)p, x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  else
    __hip_atomic_store((gu64*)p, x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void put_granule(unsigned long long* p, unsigned tag, unsigned v, bool local) {
  store_granule(p, ((unsigned long long)tag << 32) | v, local);
}
__device__ __forceinline__ unsigned long long get_granule(const unsigned long long* p) {
  return __hip_atomic_load((gu64*)p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// Sweep N granules per lane (stride XCH_NTH, starting at this lane) until every tag == tag; the values
// go to dst(q, granule) in ascending q. On timeout the kernel records `fail` and stops waiting (the results
// are then garbage, the launch still terminates); the caller folds `fail` into a persistent status
// word right after the launch (b2p_gru_mc_status), which the host checks at its next sync and raises.
template <int N, typename Tag, typename Dst>
__device__ __forceinline__ void sweep(const unsigned long long* slot, Tag tag_ok, Dst dst, int* fail, bool& dead) {
  static_assert(N <= 64, "one 64-bit pending mask per lane");
  const int lane = threadIdx.x;
  unsigned long long v[N];
  unsigned long long miss = 0;   // granules of this lane not yet seen with this step's tag
#pragma unroll
  for (int k = 0; k < N; ++k) {
    v[k] = get_granule(slot + k * XCH_NTH + lane);
    if (!tag_ok(v[k])) miss |= 1ull << k;
  }
  for (unsigned spins = 0; __any(miss != 0) && !dead; ++spins) {
    if (spins > SPIN_MAX) {
      dead = true;
      if (lane == 0) __hip_atomic_store(fail, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      break;
    }
    __builtin_amdgcn_s_sleep(1);
    // every missing granule is re-read before any is looked at: one L2 round trip per pass, not one per
    // granule (a granule seen with this step's tag keeps its value until the slot's parity comes round
    // again, which needs this member's next publish first)
#pragma unroll
    for (int k = 0; k < N; ++k)
      if (miss & (1ull << k)) v[k] = get_granule(slot + k * XCH_NTH + lane);
#pragma unroll
    for (int k = 0; k < N; ++k)
      if ((miss & (1ull << k)) && tag_ok(v[k])) miss &= ~(1ull << k);
  }
#pragma unroll
  for (int k = 0; k < N; ++k) dst(k * XCH_NTH + lane, v[k]);
}

// the sweep over a slot's NGR granules per lane, SW of them per call (one call when SW == NGR): the sweep keeps
// every granule it polls in registers, which the H = 1024 kernels cannot spare for all NGR at once. dst still
// sees the granules in ascending q.
template <int NGR, int SW, typename Tag, typename Dst>
__device__ __forceinline__ void sweep_parts(const unsigned long long* slot, Tag tag_ok, Dst dst, int* fail, bool& dead) {
  static_assert(NGR % SW == 0, "whole parts");
  if constexpr (SW == NGR) {
    sweep<NGR>(slot, tag_ok, dst, fail, dead);
  } else {
#pragma unroll
    for (int c = 0; c < NGR / SW; ++c)
      sweep<SW>(slot + c * SW * XCH_NTH, tag_ok, [&](int q, unsigned long long x) { dst(q + c * SW * XCH_NTH, x); }, fail,
                dead);
  }
}

// recurrence (d, bg) and member of this block; false for blocks with no work
__device__ __forceinline__ bool place(int P, int ngroups, int& d, int& bg, int& m, int nbg) {
  int g;
  if (ngroups <= 8) {   // members of a group on blocks with equal blockIdx % 8
    g = blockIdx.x % 8;
    m = blockIdx.x / 8;
    if (g >= ngroups) return false;
  } else {
    g = blockIdx.x % ngroups;
    m = blockIdx.x / ngroups;
  }
  d = g / nbg;
  bg = g % nbg;
  return m < P;
}

// the grid place() expects
inline int grid_blocks(int P, int ngroups) { return ngroups <= 8 ? 8 * P : ngroups * P; }

// Are all P members of this recurrence on one XCD? Each member publishes its XCC id once (sc1), every
// member reads all of them; the answer is uniform across the group, so the group agrees on the store
// flavour of every later granule. Placement is never assumed: any member elsewhere -> sc1 stores.
__device__ __forceinline__ bool same_xcd(unsigned long long* ids, int P, int m, int* fail, bool& dead) {
  __shared__ int all_same;
  unsigned xcc;
  asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
  xcc &= 0xFu;
  if (threadIdx.x == 0) {
    __hip_atomic_store((gu64*)(ids + m), (1ull << 32) | xcc, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    all_same = 1;
  }
  __syncthreads();
  if (threadIdx.x < 64) {   // one wave polls the P ids
    unsigned long long x = 0;
    bool ok = threadIdx.x >= P;
    for (unsigned spins = 0; !__all(ok); ++spins) {
      if (spins > SPIN_MAX) {
        dead = true;
        if (threadIdx.x == 0) __hip_atomic_store(fail, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        break;
      }
      if (!ok) {
        x = get_granule(ids + threadIdx.x);
        ok = (unsigned)(x >> 32) == 1u;
      }
    }
    if (threadIdx.x < P && (unsigned)x != xcc) all_same = 0;
  }
  __syncthreads();
  const bool same = all_same != 0 && !dead;
  if (same && m == 0 && threadIdx.x == 0) atomicAdd(fail + 1, 1);   // diagnostic: groups on one XCD
  return same;
}

// every polled word (tags) and the fail flag are zeroed before every launch, by a kernel (a node of
// a captured graph, replayed first): granules of a previous launch never match this launch's tags.
// (A captured hipMemsetAsync node was observed leaving foreign bytes in the first 16 bytes of the
// block on replays after the first, ROCm 7.2.)
__global__ void zero16_k(uint4* __restrict__ p, int64_t n16) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n16; i += (int64_t)gridDim.x * blockDim.x)
    p[i] = make_uint4(0u, 0u, 0u, 0u);
}
inline void launch_zero16(void* p, int64_t bytes, hipStream_t st) {
  const int64_t n16 = bytes / 16;
  const int64_t nb = (n16 + 255) / 256;
  hipLaunchKernelGGL(zero16_k, dim3((unsigned)(nb < 1024 ? nb : 1024)), dim3(256), 0, st, (uint4*)p, n16);
}

// workspace of one launch: [fail word block 16 B][ids: groups x IDS_PER_GROUP x 8 B][exchange slots]
struct XchWs { int* fail; unsigned long long* ids; unsigned long long* xch; };
// zeroes the first zero_bytes of ws on st and carves it (the slots start hdr_bytes in)
inline int xch_prepare(void* ws, int64_t hdr_bytes, int64_t zero_bytes, hipStream_t st, XchWs* w) {
  launch_zero16(ws, zero_bytes, st);
  B2P_CHECK_LAUNCH();
  char* p = reinterpret_cast<char*>(ws);
  *w = {reinterpret_cast<int*>(p), reinterpret_cast<unsigned long long*>(p + 16),
        reinterpret_cast<unsigned long long*>(p + hdr_bytes)};
  return 0;
}

// Argument checks common to the four entry points (who: the name their error texts carry; sizes: the hidden
// sizes they take). 0: go on, 1: error set, -1: nothing to do (empty batch or time).
inline int xch_check_args(const char* who, bool pointers, bool h_ok, int64_t H, const char* sizes, int ndir,
                          const void* ws, int64_t B, int64_t T) {
  B2P_CHECK_ARG(pointers && ws, "%s: NULL pointer", who);
  B2P_CHECK_ARG(h_ok, "%s: hidden size %lld unsupported (%s)", who, (long long)H, sizes);
  B2P_CHECK_ARG(ndir == 1 || ndir == 2, "%s: ndir must be 1 or 2", who);
  B2P_CHECK_ARG((((uintptr_t)ws) & 15u) == 0, "%s: workspace must be 16-byte aligned", who);
  return B <= 0 || T <= 0 ? -1 : 0;
}
}  // namespace
