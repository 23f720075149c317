// Shared helpers of the label-map units (instances, boundary, curves, watershed, pairs, sdf, cellprops, hull,
// neighbors, evalpath): launch sizing, cleared buffers, the plane-stack shape rule, integer wave reductions, the flag scan that
// numbers things in raster order, and the open-addressing hash table.  All of it is integer and exact.
//
// Debug build: table_update asserts, and EUNET_DASSERT writes to the including unit's g_eunet_dbg, which
// EUNET_DEBUG_UNIT(tag) defines further down in the unit.  This header declares that word itself, so every unit
// includes it right after common.h, before its EUNET_DEBUG_UNIT line, and a unit that names no debug unit (curves,
// evalpath) still compiles: the asserting code is a template it never instantiates.  A failing assertion of this
// header is reported under the including unit's tag with the line number of this file.
#pragma once
#include "common.h"

#ifdef EUNET_DEBUG
extern __device__ unsigned g_eunet_dbg[2];
#endif

constexpr int LM_NT = 256;  // the block size of every launch sized or scanned here

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------
// blocks of LM_NT threads for n threads, at most cap and at least one
inline unsigned grid_for(long long n, long long cap) {
  long long b = (n + LM_NT - 1) / LM_NT;
  if (b > cap) b = cap;
  return (unsigned)(b < 1 ? 1 : b);
}

inline bool fill_async(void* p, int byte, size_t bytes, hipStream_t s, const char* what) {
  if (hipMemsetAsync(p, byte, bytes, s) != hipSuccess) {
    eunet::set_error("%s: memset failed", what);
    return false;
  }
  return true;
}

// a stack of p planes of h x w pixels: p 1..65535 (a grid dimension), h and w 1..EUNET_EDT_MAX_SIDE;
// bound_pixels: also p h w < 2^31, for the units that index the whole stack with an int
inline bool plane_stack_ok(int p, int h, int w, bool bound_pixels) {
  return p >= 1 && p <= 65535 && h >= 1 && h <= EUNET_EDT_MAX_SIDE && w >= 1 && w <= EUNET_EDT_MAX_SIDE &&
         (!bound_pixels || (long long)p * h * w < (1ll << 31));
}

// ---------------------------------------------------------------------------
// integer wave reductions (wave64), next to common.h's wave_sum(float)
// ---------------------------------------------------------------------------
__device__ __forceinline__ int wave_sum(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ unsigned wave_sum(unsigned v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
__device__ __forceinline__ unsigned long long wave_sum(unsigned long long v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}
// the sum of 64 values that may pass 2^32 only in the last step: 32-bit shuffles for five steps (32 lanes of v <=
// 2^26 stay <= 2^31), 64 bits for the sixth
__device__ __forceinline__ unsigned long long wave_sum_wide(unsigned v) {
#pragma unroll
  for (int o = 1; o < 32; o <<= 1) v += __shfl_xor(v, o, 64);
  return (unsigned long long)v + (unsigned long long)__shfl_xor(v, 32, 64);
}
__device__ __forceinline__ int wave_max(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const int t = __shfl_xor(v, o, 64);
    v = t > v ? t : v;
  }
  return v;
}
__device__ __forceinline__ unsigned wave_max(unsigned v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned t = __shfl_xor(v, o, 64);
    v = t > v ? t : v;
  }
  return v;
}

// ---------------------------------------------------------------------------
// numbering flagged pixels 1..n in raster order, in three launches: per-block counts of LM_NT consecutive pixels
// (the unit's count kernel), one block per plane scanning its counts (scan_block_counts_kernel), per-block ranks
// (the unit's rank kernel).  The unit's two kernels differ only in the flag they pass.
// ---------------------------------------------------------------------------
// the number of set flags on the threads before this one in the block, *total = in the whole block.  Every thread
// of a block of LM_NT calls it; the second barrier lets a caller scan again at once.
__device__ __forceinline__ int block_exclusive_scan_flag(bool flag, int* total) {
  static_assert(LM_NT % 64 == 0, "whole waves");
  __shared__ int wave_tot[LM_NT / 64];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const unsigned long long bal = __ballot(flag);
  const int before = __popcll(bal & ((1ull << lane) - 1ull));
  if (lane == 0) wave_tot[wv] = __popcll(bal);
  __syncthreads();
  int off = 0, tot = 0;
#pragma unroll
  for (int i = 0; i < LM_NT / 64; ++i) {
    if (i < wv) off += wave_tot[i];
    tot += wave_tot[i];
  }
  __syncthreads();
  *total = tot;
  return off + before;
}

namespace {  // a kernel of the including unit, like its own

// grid (p): block_count[plane][0..nbp) -> exclusive offsets in place, total -> counts[plane].  A template, so that
// only the units that launch it carry it.
template <int NT>
__global__ __launch_bounds__(NT) void scan_block_counts_kernel(int* block_count_all, int nbp, int32_t* counts) {
  __shared__ int buf[NT];
  __shared__ int carry;
  int* block_count = block_count_all + (long long)blockIdx.x * nbp;
  if (threadIdx.x == 0) carry = 0;
  __syncthreads();
  for (int base = 0; base < nbp; base += NT) {
    const int i = base + threadIdx.x;
    const int v = i < nbp ? block_count[i] : 0;
    buf[threadIdx.x] = v;
    __syncthreads();
    for (int o = 1; o < NT; o <<= 1) {  // Hillis-Steele inclusive scan, log2(NT) static steps
      const int t = threadIdx.x >= o ? buf[threadIdx.x - o] : 0;
      __syncthreads();
      buf[threadIdx.x] += t;
      __syncthreads();
    }
    if (i < nbp) block_count[i] = carry + buf[threadIdx.x] - v;
    __syncthreads();
    if (threadIdx.x == 0) carry += buf[NT - 1];
    __syncthreads();
  }
  if (threadIdx.x == 0) counts[blockIdx.x] = carry;
}

}  // namespace

// ---------------------------------------------------------------------------
// open-addressing hash table of 64-bit keys and int32 values, filled by one launch
// ---------------------------------------------------------------------------
constexpr int MAX_PROBE = 64;                // slots an insert looks at before it reports the table as full
constexpr unsigned long long EMPTY = ~0ull;  // the key of a free slot: no caller's key has it

struct Table {
  unsigned long long* keys;
  int32_t* vals;
  unsigned mask;   // capacity - 1, the capacity a power of two
  int shift;       // 64 - log2(capacity)
  int probes;      // min(capacity, MAX_PROBE)
  int* overflow;
};

// what an insert does to the value of its key's slot (cleared to 0)
struct TableAdd {
  static __device__ __forceinline__ void apply(int32_t* slot, int val) { atomicAdd(slot, val); }
};
struct TableMax {
  static __device__ __forceinline__ void apply(int32_t* slot, int val) { atomicMax(slot, val); }
};

// vals[slot of key] = Op(itself, val).  Linear probing; a slot is claimed by the compare-and-swap that finds it
// empty, and a key never leaves its slot, so two lanes with the same key meet in the same slot whatever their
// order.  An insert that finds `probes` slots taken by other keys counts itself in *overflow and stores nothing:
// the host then reruns the pass with a table twice as large.
template <class Op>
__device__ __forceinline__ void table_update(const Table& t, unsigned long long key, int val) {
  unsigned slot = (unsigned)((key * 0x9E3779B97F4A7C15ull) >> t.shift) & t.mask;
  for (int probe = 0; probe < t.probes; ++probe) {
    EUNET_DASSERT(slot <= t.mask);
    const unsigned long long old = atomicCAS(t.keys + slot, EMPTY, key);
    if (old == EMPTY || old == key) {
      Op::apply(t.vals + slot, val);
      return;
    }
    slot = (slot + 1u) & t.mask;
  }
  atomicAdd(t.overflow, 1);
}

// checks the capacity, clears keys (to EMPTY), vals and *overflow on the stream and fills *t
inline int table_init(const char* what, int64_t* keys, int32_t* vals, long long capacity, int32_t* overflow,
                      hipStream_t s, Table* t) {
  EUNET_REQUIRE(capacity >= 2 && capacity <= (1ll << 30) && (capacity & (capacity - 1)) == 0,
                "%s: the capacity must be a power of two in 2..2^30 (got %lld)", what, capacity);
  if (!fill_async(keys, 0xff, sizeof(int64_t) * (size_t)capacity, s, what) ||
      !fill_async(vals, 0, sizeof(int32_t) * (size_t)capacity, s, what) ||
      !fill_async(overflow, 0, sizeof(int32_t), s, what))
    return EUNET_ERR_HIP;
  int log2cap = 0;
  while ((1ll << log2cap) < capacity) ++log2cap;
  *t = {(unsigned long long*)keys, vals, (unsigned)(capacity - 1), 64 - log2cap,
        (int)(capacity < MAX_PROBE ? capacity : MAX_PROBE), overflow};
  return EUNET_OK;
}
