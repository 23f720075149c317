// Shared skeleton of the per-pixel loss units (loss, bce_dice, the boundary loss of sdf): fp32 [N][K][H][W] logits
// streamed once per direction.  Forward: one block of PL_NT threads per (sample, tile of PL_LPIX pixels) sums
// NV values per thread, pl_block_row writes the tile's partial row, and a single block takes each sample's fp64 sum
// of the rows with pl_sample_sum (fixed order: deterministic).  Backward: one thread per pixel, or per group of 4
// on the 16-byte path.  Here: the shape rule of include/eunet.h ("per-pixel losses"), the sizes of sums and
// workspace, the 16-byte eligibility test, the pixel visit, the two reductions, the plane loads and stores, and the
// per-pixel softmax and sigmoid.  What a pixel contributes stays in the unit.
//
// Debug build: the visits assert their bounds through the including unit's g_eunet_dbg, which EUNET_DEBUG_UNIT(tag)
// defines further down in the unit.  This header declares that word itself, so a unit includes it right after
// common.h, before its EUNET_DEBUG_UNIT line.  A failing assertion of this header is reported under the including
// unit's tag with the line number of this file.
#pragma once
#include <initializer_list>

#include "common.h"

#ifdef EUNET_DEBUG
extern __device__ unsigned g_eunet_dbg[2];
#endif

constexpr int PL_NT = 256;     // the block size of every launch of these units
constexpr int PL_LPIX = 1024;  // pixels per partial tile: 4 per thread

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------
// the shape rule of every loss entry point: the finalize block holds 64 samples' terms in LDS, the kernels are
// built for K = 1..3 and index a plane with an int that may run one tile past its end
inline bool pl_shape_ok(int n, int k, int h, int w) {
  return n >= 1 && n <= 64 && k >= 1 && k <= 3 && h > 0 && w > 0 && (long long)h * w < (1ll << 31) - PL_LPIX;
}
#define PL_SHAPE_RULE "N 1..64, K 1..3, H > 0, W > 0, H*W < 2^31 - 1024"

// per-class I / S / T and three more: what loss and bce_dice sum per sample
constexpr int pl_nv(int k) { return 3 + 3 * k; }
inline int pl_tiles(int hw) { return cdiv(hw, PL_LPIX); }
// [N][nv] per-sample sums and two batch words
inline int pl_sums_len(int n, int nv) { return n * nv + 2; }
// one row of nv floats per (sample, tile)
inline size_t pl_workspace_bytes(int n, int h, int w, int nv) {
  return (size_t)n * pl_tiles(h * w) * nv * sizeof(float);
}

// the 16-byte path: planes and 4-pixel groups start on 16 bytes (a null optional pointer counts as aligned)
inline bool pl_vec_ok(int hw, std::initializer_list<const void*> ptrs) {
  bool ok = hw % 4 == 0;
  for (const void* p : ptrs) ok = ok && (uintptr_t)p % 16 == 0;
  return ok;
}

// blocks of the backward launch: one thread per pixel, or per 4 on the 16-byte path
inline unsigned pl_bwd_grid(int n, int hw, bool vec) {
  const long long threads = (long long)n * hw / (vec ? 4 : 1);
  return (unsigned)((threads + PL_NT - 1) / PL_NT);
}

// ---------------------------------------------------------------------------
// planes: one pixel (scalar) or 4 consecutive pixels (one 16-byte access per plane) of K planes HW elements apart
// ---------------------------------------------------------------------------
// p: the pixel within the plane, where base is the sample's first plane
template <int K>
__device__ __forceinline__ void pl_load(const float* base, int HW, float (&x)[K], int p = 0) {
#pragma unroll
  for (int c = 0; c < K; ++c) x[c] = base[(long long)c * HW + p];
}
template <int K>
__device__ __forceinline__ void pl_store(float* base, int HW, const float (&x)[K]) {
#pragma unroll
  for (int c = 0; c < K; ++c) base[(long long)c * HW] = x[c];
}
template <int K>
__device__ __forceinline__ void pl_load4(const float* base, int HW, f32x4 (&v)[K], int p = 0) {
#pragma unroll
  for (int c = 0; c < K; ++c) v[c] = *reinterpret_cast<const f32x4*>(base + (long long)c * HW + p);
}
template <int K>
__device__ __forceinline__ void pl_store4(float* base, int HW, const f32x4 (&v)[K]) {
#pragma unroll
  for (int c = 0; c < K; ++c) *reinterpret_cast<f32x4*>(base + (long long)c * HW) = v[c];
}
// 4 consecutive int64 targets: two 16-byte loads
__device__ __forceinline__ void pl_load4(const int64_t* p, int64_t (&t)[4]) {
  typedef long long i64x2 __attribute__((ext_vector_type(2)));
  const i64x2 t01 = *reinterpret_cast<const i64x2*>(p);
  const i64x2 t23 = *reinterpret_cast<const i64x2*>(p + 2);
  t[0] = t01[0], t[1] = t01[1], t[2] = t23[0], t[3] = t23[1];
}
// pixel j of a group of 4
template <int K>
__device__ __forceinline__ void pl_px(const f32x4 (&v)[K], int j, float (&x)[K]) {
#pragma unroll
  for (int c = 0; c < K; ++c) x[c] = v[c][j];
}

// ---------------------------------------------------------------------------
// forward: grid (tiles, N), PL_NT threads
// ---------------------------------------------------------------------------
// the pixels of tile blockIdx.x of a sample of HW pixels: group(p) for the first pixel p of every group of PER this
// thread owns.  VEC: the 4 pixels p0 + 4 tid + j; scalar: the pixels p0 + tid + 256 i.
template <bool VEC, class F>
__device__ __forceinline__ void pl_tile_visit(int HW, F&& group) {
  const int p0 = blockIdx.x * PL_LPIX;
  const int p1 = min(HW, p0 + PL_LPIX);
  if constexpr (VEC) {  // HW % 4 == 0: every plane and every 4-pixel group starts on 16 bytes
    const int p = p0 + threadIdx.x * 4;
    if (p < p1) {
      EUNET_DASSERT(p + 3 < HW);
      group(p);
    }
  } else {
    for (int p = p0 + threadIdx.x; p < p1; p += PL_NT) {
      EUNET_DASSERT(p < HW);
      group(p);
    }
  }
}

// the block's sums of acc[] -> the partial row of (sample blockIdx.y, tile blockIdx.x) of part [N][tiles][NV]: in
// the wave, then the four waves in order
template <int NV>
__device__ __forceinline__ void pl_block_row(const float (&acc)[NV], float* part) {
  static_assert(PL_NT == 256, "four waves");
  __shared__ float red[4][NV];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const float s = wave_sum(acc[i]);
    if (lane == 0) red[wv][i] = s;
  }
  __syncthreads();
  if (tid < NV)
    part[((long long)blockIdx.y * gridDim.x + blockIdx.x) * NV + tid] =
        red[0][tid] + red[1][tid] + red[2][tid] + red[3][tid];
}

// One 256-thread block: the threads stride over sample n's tile partials (fp64), a fixed-order LDS tree combines
// them (deterministic), v[] holds the sums in thread 0.  It can be called again at once: after the tree's last barrier
// only thread 0 reads, and only the slot that it alone writes.
template <int NV>
__device__ __forceinline__ void pl_sample_sum(const float* part, int tiles, int n, double (&v)[NV]) {
  __shared__ double red[256][NV];
  const int tid = threadIdx.x;
#pragma unroll
  for (int i = 0; i < NV; ++i) v[i] = 0.0;
  for (int t = tid; t < tiles; t += 256)
#pragma unroll
    for (int i = 0; i < NV; ++i) v[i] += (double)part[((long long)n * tiles + t) * NV + i];
#pragma unroll
  for (int i = 0; i < NV; ++i) red[tid][i] = v[i];
  __syncthreads();
  for (int off = 128; off > 0; off >>= 1) {
    if (tid < off)
#pragma unroll
      for (int i = 0; i < NV; ++i) red[tid][i] += red[tid + off][i];
    __syncthreads();
  }
  if (tid == 0)
#pragma unroll
    for (int i = 0; i < NV; ++i) v[i] = red[0][i];
}

// ---------------------------------------------------------------------------
// backward: pl_bwd_grid blocks of PL_NT threads
// ---------------------------------------------------------------------------
// this thread's group of PER pixels (HW % PER == 0, so a group never straddles two samples): its first pixel as
// id in [0, N HW) and as (sample n, pixel p); false for a thread past the end
template <int PER>
__device__ __forceinline__ bool pl_bwd_split(int N, int HW, long long& id, int& n, int& p) {
  id = ((long long)blockIdx.x * PL_NT + threadIdx.x) * PER;
  const long long total = (long long)N * HW;
  if (id >= total) return false;
  EUNET_DASSERT(id + PER <= total);
  n = (int)(id / HW);
  p = (int)(id - (long long)n * HW);
  EUNET_DASSERT(n < N && p + PER <= HW);
  return true;
}

// ---------------------------------------------------------------------------
// per pixel
// ---------------------------------------------------------------------------
// the max-subtracted softmax of one pixel; m = max x, lse_m = log sum exp(x - m)
template <int K>
__device__ __forceinline__ void softmax_px(const float (&x)[K], float (&p)[K], float& m, float& lse_m) {
  m = x[0];
#pragma unroll
  for (int c = 1; c < K; ++c) m = fmaxf(m, x[c]);
  float s = 0.f;
#pragma unroll
  for (int c = 0; c < K; ++c) {
    p[c] = expf(x[c] - m);
    s += p[c];
  }
  const float inv = 1.f / s;
#pragma unroll
  for (int c = 0; c < K; ++c) p[c] *= inv;
  lse_m = logf(s);
}
template <int K>
__device__ __forceinline__ void softmax_px(const float (&x)[K], float (&p)[K]) {
  float m, lse_m;
  softmax_px<K>(x, p, m, lse_m);
}

// sig(x), sig(-x), sp(x), sp(-x) from one exp: no overflow and no cancellation at +-100
struct Sig {
  float p, q, spp, spn;
};
template <bool WITH_SP>
__device__ __forceinline__ Sig sigmoid_terms(float x) {
  const float e = expf(-fabsf(x));
  const float r = 1.f / (1.f + e);
  const float hi = r, lo = e * r;
  Sig s;
  s.p = x >= 0.f ? hi : lo;
  s.q = x >= 0.f ? lo : hi;
  if (WITH_SP) {
    const float l = log1pf(e);
    s.spp = fmaxf(x, 0.f) + l;
    s.spn = fmaxf(-x, 0.f) + l;
  } else {
    s.spp = s.spn = 0.f;
  }
  return s;
}
