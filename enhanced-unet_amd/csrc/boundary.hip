// Exact Euclidean distance transform and the one statistics pass behind the contour metrics.
//
// Reference: visualization.py:1687-1751 (plot_boundary_accuracy: a boundary and an interior IoU per image and class,
// on the host with scipy.ndimage morphology).  The metrics the field reports (Hausdorff distance, HD95, average
// symmetric surface distance, surface Dice, boundary F1, Boundary IoU) all rest on the squared distance to the
// nearest contour pixel, which is built here exactly, in integers, for whole images:
//   edt_cols_kernel    one thread per column: a down and an up sweep give the vertical distance to the nearest
//                      site, squared; the site predicate is evaluated from the int64 map, no site mask is written
//   edt_rows_kernel    one block per row: D(x) = min_j g(j) + (x - j)^2 with the row of g staged whole in LDS (so the
//                      pass runs in place); each pixel scans outward from j = x and stops once (x - j)^2 >= its best
//   refrows_kernel     the reference's two sets (a 13-pixel L1 diamond per pixel), counted per image
//   boundary_stats_kernel  per class: the histogram of edge-to-edge squared distances in both directions, their
//                      maximum and fixed-point sum, and the Boundary-IoU band counts
// Every loop is bounded by the shapes, no block waits on another, every statistic is an integer and order-free.
// The contract is in include/eunet.h (eunet_edt_sq, eunet_boundary_stats).
#include <math.h>

#include "common.h"
#include "labelmap.h"

EUNET_DEBUG_UNIT(boundary)

namespace {

constexpr int COL_NT = 64;    // a wave per block: a 1024-wide map of 3 values still spreads over 51 CUs
constexpr int COL_W = COL_NT - 2;  // columns a block writes: its first and last lane hold the neighbouring columns
constexpr int COL_CH = 16;    // rows per chunk of the column sweeps (COL_CH + 2 bits of an unsigned mask)
constexpr int ROW_NT = 256;
constexpr int NT = 256;
constexpr unsigned NONE = (unsigned)EUNET_EDT_NONE;
constexpr int MAX_BLOCKS = 2048;  // what the two counting kernels aim at in all

struct Vals {
  long long v[EUNET_EDT_MAX_VALUES];
};
struct Radii {
  unsigned r2[EUNET_BOUNDARY_MAX_RADII];
};

// One sample's map as the kernels see it: where gate (optional) holds ign the map reads as ign too -- the ignore
// rule of eunet_boundary_stats, applied in the predicate.
struct MapView {
  const int64_t* m;
  const int64_t* gate;
  long long ign;
  int h, w;
  __device__ __forceinline__ long long at(int y, int x) const {
    EUNET_DASSERT(y >= 0 && y < h && x >= 0 && x < w);
    const long long i = (long long)y * w + x;
    long long val = (long long)m[i];
    if (gate) val = (long long)gate[i] == ign ? ign : val;
    return val;
  }
  // x in R_v; a position outside the image is in no region.  The load is unconditional, from the clamped
  // position, so that a run of these tests issues its loads back to back instead of one branch at a time.
  __device__ __forceinline__ bool in(int y, int x, long long v) const {
    const bool inside = y >= 0 && y < h && x >= 0 && x < w;
    const int yc = y < 0 ? 0 : (y >= h ? h - 1 : y), xc = x < 0 ? 0 : (x >= w ? w - 1 : x);
    return (at(yc, xc) == v) & inside;
  }
};

// grid (ceil(w / COL_W), nv, n): thread = one column of one (sample, value) plane; lanes 0 and 63 of the wave read
// the columns left and right of the block's COL_W and write nothing, so that the edge mode gets a pixel's horizontal
// neighbours from the neighbouring lanes (one map load per pixel, not three).  The down sweep leaves the
// distance to the nearest site at or above (NONE: none so far), the up sweep combines it with the one below and
// writes the square.  A column holds at most 8192 pixels, so a distance fits and its square is < 2^26.
// Both sweeps go in chunks of COL_CH rows: a chunk's loads are issued together, then the serial recurrence runs in
// registers (one load per step would leave the thread waiting on memory 2 h times).
template <int MODE>
__global__ __launch_bounds__(COL_NT) void edt_cols_kernel(const int64_t* __restrict__ labels,
                                                          const int64_t* __restrict__ gate, long long ign, int h, int w,
                                                          Vals vals, int nv, int32_t* __restrict__ out) {
  const int x = blockIdx.x * COL_W + (int)threadIdx.x - 1;  // -1 and w are read as "outside every region"
  const bool writer = threadIdx.x >= 1 && threadIdx.x <= COL_W && x < w;  // no early return: the shuffles need the wave
  const int j = blockIdx.y, img = blockIdx.z;
  const long long v = vals.v[j];
  const long long hw = (long long)h * w;
  const MapView mv = {labels + img * hw, gate ? gate + img * hw : nullptr, ign, h, w};
  unsigned* o = (unsigned*)out + ((long long)img * nv + j) * hw + (writer ? x : 0);

  unsigned d = NONE;
  for (int y0 = 0; y0 < h; y0 += COL_CH) {
    unsigned sites = 0u;  // bit i: (y0 + i, x) is a site
    if (MODE == EUNET_EDT_EDGE) {
      unsigned cen = 0u;  // bit i: (y0 - 1 + i, x) in R_v
#pragma unroll
      for (int i = 0; i < COL_CH + 2; ++i) cen |= (unsigned)mv.in(y0 - 1 + i, x, v) << i;
      // both horizontal neighbours in R_v, from the lanes of the columns x - 1 and x + 1 (writers have both)
      const unsigned side = __shfl_up(cen, 1, 64) & __shfl_down(cen, 1, 64);
      sites = (cen >> 1) & ~(cen & (cen >> 2) & (side >> 1));  // in the region, and not all four neighbours in it
    } else {
#pragma unroll
      for (int i = 0; i < COL_CH; ++i) sites |= (unsigned)mv.in(y0 + i, x, v) << i;
      if (MODE == EUNET_EDT_NE) sites = ~sites;
    }
#pragma unroll
    for (int i = 0; i < COL_CH; ++i) {
      const int y = y0 + i;
      if (writer && y < h) {
        d = ((sites >> i) & 1u) ? 0u : (d == NONE ? NONE : d + 1u);
        o[(long long)y * w] = d;
      }
    }
  }
  if (!writer) return;
  d = NONE;
  for (int y1 = h; y1 > 0; y1 -= COL_CH) {  // the rows y1 - 1 down to y1 - COL_CH
    unsigned t[COL_CH];
#pragma unroll
    for (int i = 0; i < COL_CH; ++i) {
      const int y = y1 - 1 - i;
      t[i] = o[(long long)(y < 0 ? 0 : y) * w];
    }
#pragma unroll
    for (int i = 0; i < COL_CH; ++i) {
      const int y = y1 - 1 - i;
      if (y >= 0) {
        d = t[i] == 0u ? 0u : (d == NONE ? NONE : d + 1u);
        const unsigned mn = t[i] < d ? t[i] : d;
        EUNET_DASSERT(mn == NONE || mn < (unsigned)h);
        o[(long long)y * w] = mn == NONE ? NONE : mn * mn;
      }
    }
  }
}

// grid (h, nv, n): block = one row of one plane, in place.  g (<= 2^26, or NONE) + r^2 (< 2^26) cannot wrap in 32
// unsigned bits, and a NONE term never wins a minimum against a finite one.  A row without a finite g stays NONE
// (a sample without a site: every row is such a row) and is not scanned.
__global__ __launch_bounds__(ROW_NT) void edt_rows_kernel(int32_t* out, int w) {
  extern __shared__ __attribute__((aligned(16))) unsigned g[];
  unsigned* row =
      (unsigned*)out + (((long long)blockIdx.z * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x) * (long long)w;
  int any = 0;
  for (int x = threadIdx.x; x < w; x += ROW_NT) {
    const unsigned t = row[x];
    g[x] = t;
    any |= t != NONE;
  }
  if (!__syncthreads_or(any)) return;
  for (int x = threadIdx.x; x < w; x += ROW_NT) {
    unsigned best = g[x];
    const int reach = x > w - 1 - x ? x : w - 1 - x;
    for (int r = 1; r <= reach; ++r) {
      const unsigned r2 = (unsigned)r * (unsigned)r;
      if (r2 >= best) break;
      if (x - r >= 0) {
        const unsigned c = g[x - r] + r2;
        best = c < best ? c : best;
      }
      if (x + r < w) {
        const unsigned c = g[x + r] + r2;
        best = c < best ? c : best;
      }
    }
    EUNET_DASSERT(best <= NONE);
    row[x] = best;
  }
}

// floor(2^16 sqrt(d2)) = the integer square root of N = d2 2^32 (d2 < 2^28, so N < 2^60 is exact in a double and
// the rounded double root is within 1 of it)
__device__ __forceinline__ unsigned long long isqrt_q16(unsigned d2) {
  const unsigned long long n = (unsigned long long)d2 << 32;
  unsigned long long s = (unsigned long long)sqrt((double)n);
  if (s * s > n) --s;
  if ((s + 1) * (s + 1) <= n) ++s;
  return s;
}

// The 13 positions of the radius-2 L1 diamond; the first 5 are the radius-1 diamond.
__constant__ const signed char DIAMOND[13][2] = {{0, 0},  {-1, 0}, {1, 0},  {0, -1}, {0, 1}, {-2, 0}, {2, 0},
                                                 {0, -2}, {0, 2},  {-1, -1}, {-1, 1}, {1, -1}, {1, 1}};

// grid (gx, 1, n): thread = pixels of one image, all k classes at once.  Per class and map, bit i of a mask says
// that diamond position i is inside the image and of the class.  cnt[c][row][pred, gt, both].
__global__ __launch_bounds__(NT) void refrows_kernel(const int64_t* pred, const int64_t* gt, int h, int w, int k,
                                                     unsigned long long* refrows) {
  __shared__ unsigned tot[18];
  if (threadIdx.x < 18) tot[threadIdx.x] = 0u;
  __syncthreads();
  const int img = blockIdx.z;
  const long long hw = (long long)h * w;
  const int64_t* maps[2] = {pred + img * hw, gt + img * hw};
  unsigned cnt[18];
#pragma unroll
  for (int i = 0; i < 18; ++i) cnt[i] = 0u;
  for (long long p = (long long)blockIdx.x * NT + threadIdx.x; p < hw; p += (long long)gridDim.x * NT) {
    const int y = (int)(p / w), x = (int)(p - (long long)y * w);
    unsigned bits[2][3] = {{0u, 0u, 0u}, {0u, 0u, 0u}};
#pragma unroll
    for (int s = 0; s < 2; ++s) {
#pragma unroll
      for (int i = 0; i < 13; ++i) {
        // an unconditional load from the clamped position (the 26 loads of a pixel go out together); a position
        // outside the image sets no bit
        const int yy = y + DIAMOND[i][0], xx = x + DIAMOND[i][1];
        const bool inside = yy >= 0 && yy < h && xx >= 0 && xx < w;
        const long long q = (long long)(yy < 0 ? 0 : (yy >= h ? h - 1 : yy)) * w + (xx < 0 ? 0 : (xx >= w ? w - 1 : xx));
        EUNET_DASSERT(q >= 0 && q < hw);
        const long long val = (long long)maps[s][q];
#pragma unroll
        for (int c = 0; c < 3; ++c) bits[s][c] |= (unsigned)((val == (long long)c) & inside) << i;
      }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      bool r0[2], r1[2];
#pragma unroll
      for (int s = 0; s < 2; ++s) {
        r0[s] = (bits[s][c] & 0x1fu) != 0u && (bits[s][c] & 0x1fu) != 0x1fu;
        r1[s] = bits[s][c] == 0x1fffu;
      }
      cnt[c * 6 + 0] += r0[0];
      cnt[c * 6 + 1] += r0[1];
      cnt[c * 6 + 2] += r0[0] && r0[1];
      cnt[c * 6 + 3] += r1[0];
      cnt[c * 6 + 4] += r1[1];
      cnt[c * 6 + 5] += r1[0] && r1[1];
    }
  }
#pragma unroll
  for (int i = 0; i < 18; ++i) {
    const unsigned s = wave_sum(cnt[i]);
    if ((threadIdx.x & 63) == 0 && s) atomicAdd(&tot[i], s);
  }
  __syncthreads();
  if ((int)threadIdx.x < 6 * k && tot[threadIdx.x])
    atomicAdd(refrows + (long long)img * k * 6 + threadIdx.x, (unsigned long long)tot[threadIdx.x]);
}

// grid (gx, k, n): block (bx, c, i) takes its share of the pixels of image i for class c.  dp / dg: the EDGE
// transforms [n][k][hw] of pred (under the ignore rule) and gt, so x is an edge pixel exactly where its own map's
// transform is 0.  A good model puts almost every edge pixel at d2 = 0: that bin, the overflow bin and the NONE bin
// are counted in registers and summed per wave; the bins 1 .. cap2 are LDS atomics of a block-private histogram.
// LDS: sums[2] (64-bit), hist [2][cap2 + 3], mx[2], bandc [8][3].  A block sees fewer than 2^27 pixels: 32-bit counts.
__global__ __launch_bounds__(NT) void boundary_stats_kernel(const int64_t* pred, const int64_t* gt,
                                                            const int32_t* dp_all, const int32_t* dg_all, int k,
                                                            long long hw, long long ign, int cap2, Radii rad, int nr,
                                                            unsigned long long* surf, unsigned long long* band) {
  extern __shared__ __attribute__((aligned(16))) unsigned long long smem[];
  unsigned long long* sums = smem;
  unsigned* hist = (unsigned*)(smem + 2);
  const int nb = cap2 + 3;
  unsigned* mx = hist + 2 * nb;
  unsigned* bandc = mx + 2;
  for (int i = threadIdx.x; i < 2 * nb + 2 + 24; i += NT) hist[i] = 0u;
  if (threadIdx.x < 2) sums[threadIdx.x] = 0ull;
  __syncthreads();

  const int c = blockIdx.y, img = blockIdx.z;
  const int64_t* p_ = pred + img * hw;
  const int64_t* g_ = gt + img * hw;
  const unsigned* dp = (const unsigned*)dp_all + ((long long)img * k + c) * hw;
  const unsigned* dg = (const unsigned*)dg_all + ((long long)img * k + c) * hw;

  unsigned zero[2] = {0u, 0u}, over[2] = {0u, 0u}, none[2] = {0u, 0u}, big[2] = {0u, 0u};
  unsigned long long sum[2] = {0ull, 0ull};
  unsigned bc[EUNET_BOUNDARY_MAX_RADII][3];
#pragma unroll
  for (int j = 0; j < EUNET_BOUNDARY_MAX_RADII; ++j) bc[j][0] = bc[j][1] = bc[j][2] = 0u;

  for (long long i = (long long)blockIdx.x * NT + threadIdx.x; i < hw; i += (long long)gridDim.x * NT) {
    const long long gv = (long long)g_[i];
    const long long pv = gv == ign ? ign : (long long)p_[i];
    const unsigned d[2] = {dp[i], dg[i]};  // the distance to the own map's edge of (pred, gt)
#pragma unroll
    for (int dir = 0; dir < 2; ++dir) {
      if (d[dir] != 0u) continue;  // not an edge pixel of this direction's map
      const unsigned d2 = d[1 - dir];
      if (d2 == 0u) ++zero[dir];
      else if (d2 == NONE) ++none[dir];
      else {
        if (d2 <= (unsigned)cap2) {
          EUNET_DASSERT(dir * nb + (int)d2 < 2 * nb);
          atomicAdd(&hist[dir * nb + d2], 1u);
        } else ++over[dir];
        big[dir] = d2 > big[dir] ? d2 : big[dir];
        sum[dir] += isqrt_q16(d2);
      }
    }
    const bool in[2] = {pv == (long long)c, gv == (long long)c};
#pragma unroll
    for (int j = 0; j < EUNET_BOUNDARY_MAX_RADII; ++j) {
      if (j < nr) {
        const bool bp = in[0] && d[0] <= rad.r2[j], bg = in[1] && d[1] <= rad.r2[j];
        bc[j][0] += bp;
        bc[j][1] += bg;
        bc[j][2] += bp && bg;
      }
    }
  }
  const bool lead = (threadIdx.x & 63) == 0;
#pragma unroll
  for (int dir = 0; dir < 2; ++dir) {
    const unsigned z = wave_sum(zero[dir]), ov = wave_sum(over[dir]), no = wave_sum(none[dir]);
    const unsigned m = wave_max(big[dir]);
    const unsigned long long s = wave_sum(sum[dir]);
    if (lead) {
      if (z) atomicAdd(&hist[dir * nb], z);
      if (ov) atomicAdd(&hist[dir * nb + cap2 + 1], ov);
      if (no) atomicAdd(&hist[dir * nb + cap2 + 2], no);
      if (m) atomicMax(&mx[dir], m);
      if (s) atomicAdd(&sums[dir], s);
    }
  }
#pragma unroll
  for (int j = 0; j < EUNET_BOUNDARY_MAX_RADII; ++j) {
    if (j < nr) {
#pragma unroll
      for (int e = 0; e < 3; ++e) {
        const unsigned s = wave_sum(bc[j][e]);
        if (lead && s) atomicAdd(&bandc[j * 3 + e], s);
      }
    }
  }
  __syncthreads();

  unsigned long long* out = surf + (long long)c * 2 * (cap2 + 5);
  for (int i = threadIdx.x; i < 2 * nb; i += NT) {
    const int dir = i / nb, b = i - dir * nb;
    if (hist[i]) atomicAdd(out + (long long)dir * (cap2 + 5) + b, (unsigned long long)hist[i]);
  }
  if (threadIdx.x < 2) {
    unsigned long long* o = out + (long long)threadIdx.x * (cap2 + 5);
    if (mx[threadIdx.x]) atomicMax(o + cap2 + 3, (unsigned long long)mx[threadIdx.x]);
    if (sums[threadIdx.x]) atomicAdd(o + cap2 + 4, sums[threadIdx.x]);
  }
  if ((int)threadIdx.x < 3 * nr && bandc[threadIdx.x])
    atomicAdd(band + (long long)c * nr * 3 + threadIdx.x, (unsigned long long)bandc[threadIdx.x]);
}

// both passes of one transform; gate / ign: the ignore rule (gate null: none)
void launch_edt(const int64_t* labels, const int64_t* gate, long long ign, int n, int h, int w, const Vals& vals, int nv,
                int mode, int32_t* out, hipStream_t s) {
  const dim3 gc((unsigned)cdiv(w, COL_W), (unsigned)nv, (unsigned)n);
  if (mode == EUNET_EDT_EQ)
    edt_cols_kernel<EUNET_EDT_EQ><<<gc, COL_NT, 0, s>>>(labels, gate, ign, h, w, vals, nv, out);
  else if (mode == EUNET_EDT_NE)
    edt_cols_kernel<EUNET_EDT_NE><<<gc, COL_NT, 0, s>>>(labels, gate, ign, h, w, vals, nv, out);
  else
    edt_cols_kernel<EUNET_EDT_EDGE><<<gc, COL_NT, 0, s>>>(labels, gate, ign, h, w, vals, nv, out);
  edt_rows_kernel<<<dim3((unsigned)h, (unsigned)nv, (unsigned)n), ROW_NT, (size_t)w * 4, s>>>(out, w);
}

// blocks along x for a counting kernel with `planes` (y, z) blocks over hw pixels: about 2048 pixels a block,
// MAX_BLOCKS in all
unsigned count_blocks(long long hw, long long planes) {
  long long gx = (hw + 8 * NT - 1) / (8 * NT);
  const long long most = MAX_BLOCKS / planes > 0 ? MAX_BLOCKS / planes : 1;
  return (unsigned)(gx > most ? most : gx);
}

}  // namespace

extern "C" {

int eunet_edt_sq(const int64_t* labels, int n, int h, int w, const int64_t* values, int nv, int mode, int32_t* out,
                 void* stream) {
  EUNET_REQUIRE(labels && values && out, "edt_sq: null pointer");
  EUNET_REQUIRE(plane_stack_ok(n, h, w, false), "edt_sq: bad shape (n 1..65535, h and w 1..%d)", EUNET_EDT_MAX_SIDE);
  EUNET_REQUIRE(nv >= 1 && nv <= EUNET_EDT_MAX_VALUES, "edt_sq: 1..%d values", EUNET_EDT_MAX_VALUES);
  EUNET_REQUIRE(mode == EUNET_EDT_EQ || mode == EUNET_EDT_NE || mode == EUNET_EDT_EDGE, "edt_sq: unknown mode %d", mode);
  EUNET_REQUIRE(((uintptr_t)labels & 7u) == 0 && ((uintptr_t)out & 3u) == 0, "edt_sq: misaligned labels / out");
  Vals vals = {};
  for (int j = 0; j < nv; ++j) vals.v[j] = (long long)values[j];
  launch_edt(labels, nullptr, 0, n, h, w, vals, nv, mode, out, (hipStream_t)stream);
  EUNET_LAUNCH_CHECK("edt_sq");
  return EUNET_OK;
}

int eunet_boundary_workspace_bytes(int n, int k, int h, int w, size_t* bytes) {
  EUNET_REQUIRE(bytes, "boundary_workspace_bytes: null pointer");
  EUNET_REQUIRE(plane_stack_ok(n, h, w, false) && k >= 1 && k <= 3,
                "boundary_workspace_bytes: bad shape (k 1..3, h and w 1..%d)", EUNET_EDT_MAX_SIDE);
  *bytes = (size_t)2 * n * k * h * w * sizeof(int32_t);
  return EUNET_OK;
}

int eunet_boundary_stats(const int64_t* pred, const int64_t* gt, int n, int h, int w, int k, int ignore_index, int cap,
                         const int* radii, int nr, int32_t* ws, int64_t* surf, int64_t* band, int64_t* refrows,
                         void* stream) {
  EUNET_REQUIRE(pred && gt && ws && surf && refrows, "boundary_stats: null pointer");
  EUNET_REQUIRE(plane_stack_ok(n, h, w, false) && k >= 1 && k <= 3,
                "boundary_stats: bad shape (n 1..65535, k 1..3, h and w 1..%d)", EUNET_EDT_MAX_SIDE);
  EUNET_REQUIRE(cap >= 1 && cap <= EUNET_BOUNDARY_MAX_CAP, "boundary_stats: cap 1..%d", EUNET_BOUNDARY_MAX_CAP);
  EUNET_REQUIRE(nr >= 0 && nr <= EUNET_BOUNDARY_MAX_RADII && (nr == 0 || (radii && band)),
                "boundary_stats: 0..%d radii (with their array and band)", EUNET_BOUNDARY_MAX_RADII);
  EUNET_REQUIRE(((uintptr_t)pred & 7u) == 0 && ((uintptr_t)gt & 7u) == 0 && ((uintptr_t)ws & 3u) == 0 &&
                    ((uintptr_t)surf & 7u) == 0 && ((uintptr_t)band & 7u) == 0 && ((uintptr_t)refrows & 7u) == 0,
                "boundary_stats: misaligned pointer");
  Radii rad = {};
  for (int j = 0; j < nr; ++j) {
    // a radius beyond the longest distance of an 8192 x 8192 map selects the whole region, as 11585 does
    EUNET_REQUIRE(radii[j] >= 0, "boundary_stats: negative radius %d", radii[j]);
    const long long r = radii[j] > 11585 ? 11585 : radii[j];
    rad.r2[j] = (unsigned)(r * r);
  }
  Vals vals = {};
  for (int c = 0; c < k; ++c) vals.v[c] = c;
  const hipStream_t s = (hipStream_t)stream;
  const long long hw = (long long)h * w;
  int32_t* dp = ws;
  int32_t* dg = ws + (long long)n * k * hw;
  const long long ign = (long long)ignore_index;
  launch_edt(pred, gt, ign, n, h, w, vals, k, EUNET_EDT_EDGE, dp, s);
  launch_edt(gt, nullptr, 0, n, h, w, vals, k, EUNET_EDT_EDGE, dg, s);
  refrows_kernel<<<dim3(count_blocks(hw, n), 1, (unsigned)n), NT, 0, s>>>(pred, gt, h, w, k,
                                                                           (unsigned long long*)refrows);
  const int cap2 = cap * cap;
  const size_t lds = 16 + (size_t)(2 * (cap2 + 3) + 2 + 24) * 4;
  boundary_stats_kernel<<<dim3(count_blocks(hw, (long long)n * k), (unsigned)k, (unsigned)n), NT, lds, s>>>(
      pred, gt, dp, dg, k, hw, ign, cap2, rad, nr, (unsigned long long*)surf, (unsigned long long*)band);
  EUNET_LAUNCH_CHECK("boundary_stats");
  return EUNET_OK;
}

}  // extern "C"
