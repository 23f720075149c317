// Per-cell measurements from label maps: the integer sums every shape, position and intensity descriptor of a cell is
// formed from (eunet/metrics.py, cell_measurements).  The definitions are in include/eunet.h ("per-cell measurements").
//   cell_init_kernel     writes both tables: zeros, and for the labels 1..n the bounding box of no pixel (w, h, -1, -1)
//                        and the intensity range of no pixel (255, 0)
//   cell_moments_kernel  one pass over the ids (and the image): a wave holds 256 consecutive pixels of one row, four
//                        per lane; the first pixel of every run of one measured id adds the run's area and moments in
//                        closed form, its bounding box and, with an image, its intensity sums and range (a segmented
//                        reduction over the lanes) to the label's row with 64-bit integer atomics
//   cell_quads_kernel    one pass over the (h + 1) (w + 1) windows of 2 x 2 pixels of the plane padded by one pixel of
//                        outside: every label of a window that is not of one value adds one to its bit-quad count
// The bounding box is kept with SIGNED 64-bit atomic min / max on the inclusive coordinates themselves (the table's
// -1 is a plain signed value; nothing is stored shifted and no pass follows).  Every loop is bounded by the shapes or
// by a constant, every result is an integer and independent of the order in which the atomics land.
#include "common.h"
#include "labelmap.h"

EUNET_DEBUG_UNIT(cellprops)

namespace {

constexpr int NT = 256;
static_assert(NT == LM_NT, "labelmap.h sizes blocks of NT");
constexpr int GRID_CAP = 4096;  // blocks of a grid-stride launch
constexpr int PV = 4;             // pixels a lane holds
constexpr int WAVE_PX = 64 * PV;  // pixels a wave holds
constexpr int GC = EUNET_CELL_GEOM_COLS;
typedef unsigned long long u64;

struct Tables {
  long long* geom;   // [p][n + 1][GC]
  long long* inten;  // [p][n + 1][c][4], null without an image
  long long rows;    // p (n + 1)
  int n;
};

__device__ __forceinline__ void add64(long long* p, long long v) { atomicAdd((u64*)p, (u64)v); }
// Always issued: reading the entry first and leaving out an atomic that cannot move it was measured slower (the
// loads of lines that atomics keep dropping from the cache cost more than the atomics they save).
__device__ __forceinline__ void min64(long long* p, long long v) {
  __hip_atomic_fetch_min(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void max64(long long* p, long long v) {
  __hip_atomic_fetch_max(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

template <int C>
__global__ __launch_bounds__(NT) void cell_init_kernel(Tables t, int h, int w) {
  const long long per = GC + 4 * C;
  const long long total = t.rows * per;
  for (long long i = (long long)blockIdx.x * NT + threadIdx.x; i < total; i += (long long)gridDim.x * NT) {
    const long long row = i / per;
    const int col = (int)(i - row * per);
    const bool label = row % (t.n + 1) != 0;  // row 0 of every plane stays zero
    EUNET_DASSERT(row >= 0 && row < t.rows && col >= 0 && col < per);
    if (col < GC) {
      long long v = 0;
      if (label) v = col == 6 ? w : col == 7 ? h : (col == 8 || col == 9) ? -1 : 0;
      t.geom[row * GC + col] = v;
    } else {
      const int k = col - GC;  // channel * 4 + (sum, sum of squares, min, max)
      t.inten[row * (4 * C) + k] = label && (k & 3) == 2 ? 255 : 0;
    }
  }
}

// the sum of x^2 over 0 <= x <= m (m >= -1): the square-pyramid number
__device__ __forceinline__ long long pyramid(long long m) { return m * (m + 1) * (2 * m + 1) / 6; }

// the reduction of a set of pixels of one channel: sum, sum of squares, min | (255 - max) << 8 kept as two minima
struct Red {
  unsigned s, q, lo, hi;  // hi holds 255 - max, so both range ends reduce with min
};
__device__ __forceinline__ Red red_id() { return {0u, 0u, 255u, 255u}; }
__device__ __forceinline__ Red red_px(unsigned v) { return {v, v * v, v, 255u - v}; }
__device__ __forceinline__ Red red_op(const Red& a, const Red& b) {
  return {a.s + b.s, a.q + b.q, a.lo < b.lo ? a.lo : b.lo, a.hi < b.hi ? a.hi : b.hi};
}
__device__ __forceinline__ Red red_down(const Red& a, int d) {
  const unsigned m = __shfl_down(a.lo | (a.hi << 8), d, 64);
  return {(unsigned)__shfl_down(a.s, d, 64), (unsigned)__shfl_down(a.q, d, 64), m & 255u, m >> 8};
}

// grid-stride over units of WAVE_PX pixels, one per wave and round: unit = (plane, row, chunk of the row).  A chunk
// never crosses a row end, so a run has one y.  Whole waves only: the shuffles and ballots need every lane; lanes past
// the row's end hold uncounted pixels (key 0) and never write, and no lane leaves before the last shuffle.  A boundary
// is a pixel whose key differs from the one before it in the chunk (the chunk's first pixel is one), as in
// pairs_kernel; a boundary with a measured id is a run head and issues the atomics of its whole run.  The key of a
// pixel is its id when that lies in 1..n and 0 otherwise: background, skipped ids and the lanes past the row.
template <typename T, int C>
__global__ __launch_bounds__(NT) void cell_moments_kernel(const T* __restrict__ ids, int p, int h, int w,
                                                          const uint8_t* __restrict__ image, Tables t,
                                                          long long* __restrict__ skipped) {
  const int cpr = (w + WAVE_PX - 1) / WAVE_PX;  // chunks per row
  const long long units = (long long)p * h * cpr;
  const long long hw = (long long)h * w;
  const int lane = threadIdx.x & 63;
  const long long wave = (long long)blockIdx.x * (NT / 64) + (threadIdx.x >> 6);
  const long long waves = (long long)gridDim.x * (NT / 64);
  for (long long u = wave; u < units; u += waves) {
    const long long prow = u / cpr;  // plane * h + y
    const int chunk = (int)(u - prow * cpr);
    const int plane = (int)(prow / h);
    const int y = (int)(prow - (long long)plane * h);
    const int x0 = chunk * WAVE_PX + lane * PV;
    const long long base = prow * w;  // of the row in ids
    int key[PV];
    unsigned skip = 0;
    {
      long long v[PV];
      const T* src = ids + base + x0;
      if (x0 + PV <= w && ((uintptr_t)src & 15u) == 0) {
        EUNET_DASSERT(base + x0 + PV <= (long long)p * hw);
        if constexpr (sizeof(T) == 4) {
          const int4 q = *reinterpret_cast<const int4*>(src);
          v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
        } else {
          const longlong2 q0 = *reinterpret_cast<const longlong2*>(src);
          const longlong2 q1 = *reinterpret_cast<const longlong2*>(src + 2);
          v[0] = q0.x; v[1] = q0.y; v[2] = q1.x; v[3] = q1.y;
        }
      } else {
#pragma unroll
        for (int j = 0; j < PV; ++j) {
          EUNET_DASSERT(x0 + j >= w || base + x0 + j < (long long)p * hw);
          v[j] = x0 + j < w ? (long long)src[j] : 0ll;
        }
      }
#pragma unroll
      for (int j = 0; j < PV; ++j) {
        const bool out = v[j] < 0 || v[j] > t.n;
        skip += out ? 1u : 0u;
        key[j] = out ? 0 : (int)v[j];
      }
    }
    // skipped pixels of the chunk: one add per wave
    skip = wave_sum(skip);
    if (lane == 0 && skip) {
      EUNET_DASSERT(plane >= 0 && plane < p);
      add64(skipped + plane, (long long)skip);
    }

    int prev = __shfl_up(key[PV - 1], 1, 64);
    unsigned bm = 0;  // bit j: pixel j of this lane is a boundary
#pragma unroll
    for (int j = 0; j < PV; ++j) {
      if ((j == 0 && lane == 0) || key[j] != prev) bm |= 1u << j;
      prev = key[j];
    }
    // the first boundary after this lane's pixels: in lane nl, at its pixel ctz(nbm)
    const u64 anyb = __ballot(bm != 0);
    const u64 above = lane == 63 ? 0ull : anyb >> (lane + 1);
    const int nl = above ? lane + __ffsll((long long)above) : lane;
    const unsigned nbm = __shfl(bm, nl, 64);
    const int beyond = above ? PV * (nl - lane - 1) + (__ffs((int)nbm) - 1) : PV * (63 - lane);

    // intensity: px[k][j] the value of channel k at pixel j; next[k] the reduction over the pixels after this lane
    // up to the next boundary (a segmented suffix scan over the lanes' leading parts, the pixels before a lane's
    // first boundary)
    Red px[C > 0 ? C : 1][PV], next[C > 0 ? C : 1];
    if constexpr (C > 0) {
      unsigned char b[PV * C];
      const long long off = (base - (long long)plane * hw + x0) * C;  // the image is shared by the planes
      const uint8_t* src = image + off;
      if (x0 + PV <= w && ((uintptr_t)src & 3u) == 0) {
        EUNET_DASSERT(off >= 0 && off + PV * C <= hw * C);
        unsigned wd[C];
#pragma unroll
        for (int k = 0; k < C; ++k) wd[k] = reinterpret_cast<const unsigned*>(src)[k];
#pragma unroll
        for (int i = 0; i < PV * C; ++i) b[i] = (unsigned char)(wd[i >> 2] >> (8 * (i & 3)));
      } else {
#pragma unroll
        for (int i = 0; i < PV * C; ++i) {
          EUNET_DASSERT(x0 + i / C >= w || (off + i >= 0 && off + i < hw * C));
          b[i] = x0 + i / C < w ? src[i] : (unsigned char)0;
        }
      }
      const int lead = bm ? __ffs((int)bm) - 1 : PV;  // pixels before this lane's first boundary
#pragma unroll
      for (int k = 0; k < C; ++k) {
        Red a = red_id();
#pragma unroll
        for (int j = 0; j < PV; ++j) {
          px[k][j] = red_px(b[j * C + k]);
          if (j < lead) a = red_op(a, px[k][j]);
        }
        next[k] = a;
      }
      bool stop = bm != 0;  // the segment ends in this lane: nothing of the lanes above is added
#pragma unroll
      for (int d = 1; d < 64; d <<= 1) {
        const bool sd = __shfl_down((int)stop, d, 64) != 0;
        const bool take = !stop && lane + d < 64;
#pragma unroll
        for (int k = 0; k < C; ++k) {
          const Red r = red_down(next[k], d);
          if (take) next[k] = red_op(next[k], r);
        }
        if (take) stop = sd;
      }
#pragma unroll
      for (int k = 0; k < C; ++k) {
        const Red r = red_down(next[k], 1);
        next[k] = lane == 63 ? red_id() : r;
      }
    }

#pragma unroll
    for (int j = 0; j < PV; ++j) {
      if (!((bm >> j) & 1u) || key[j] == 0) continue;
      const unsigned rest = bm >> (j + 1);
      const int len = rest ? __ffs((int)rest) : PV - j + beyond;
      const long long xa = x0 + j, xb = xa + len;
      EUNET_DASSERT(len >= 1 && lane * PV + j + len <= WAVE_PX && xb <= w && key[j] >= 1 && key[j] <= t.n);
      const long long row = (long long)plane * (t.n + 1) + key[j];
      EUNET_DASSERT(row >= 1 && row < t.rows);
      long long* g = t.geom + row * GC;
      const long long L = len, sx = L * (xa + xb - 1) / 2;
      add64(g + 0, L);
      add64(g + 1, sx);
      add64(g + 2, L * y);
      add64(g + 3, pyramid(xb - 1) - pyramid(xa - 1));
      add64(g + 4, L * y * y);
      add64(g + 5, sx * y);
      min64(g + 6, xa);
      min64(g + 7, y);
      max64(g + 8, xb - 1);
      max64(g + 9, y);
      if constexpr (C > 0) {
        const int last = rest ? j + len : PV;  // the run's pixels of this lane are j .. last - 1
#pragma unroll
        for (int k = 0; k < C; ++k) {
          Red a = rest ? red_id() : next[k];
#pragma unroll
          for (int i = 0; i < PV; ++i)
            if (i >= j && i < last) a = red_op(a, px[k][i]);
          long long* q = t.inten + (row * C + k) * 4;
          add64(q + 0, a.s);
          add64(q + 1, a.q);
          min64(q + 2, a.lo);
          max64(q + 3, 255u - a.hi);
        }
      }
    }
  }
}

// grid-stride over units of 64 windows, one per wave and round: unit = (plane, window row wy in 0..h, chunk of the
// w + 1 windows of the row).  The window (wy, wx) holds the pixels (wy - 1, wx - 1), (wy - 1, wx), (wy, wx - 1),
// (wy, wx); a lane loads the right column of its window and takes the left one from the lane below (lane 0 loads
// it).  Whole waves only, as above.  Pixels outside the plane and ids outside 1..n read as 0.
template <typename T>
__global__ __launch_bounds__(NT) void cell_quads_kernel(const T* __restrict__ ids, int p, int h, int w, Tables t) {
  const int cpr = (w + 1 + 63) / 64;
  const long long units = (long long)p * (h + 1) * cpr;
  const long long hw = (long long)h * w;
  const int lane = threadIdx.x & 63;
  const long long wave = (long long)blockIdx.x * (NT / 64) + (threadIdx.x >> 6);
  const long long waves = (long long)gridDim.x * (NT / 64);
  for (long long u = wave; u < units; u += waves) {
    const long long prow = u / cpr;  // plane * (h + 1) + wy
    const int chunk = (int)(u - prow * cpr);
    const int plane = (int)(prow / (h + 1));
    const int wy = (int)(prow - (long long)plane * (h + 1));
    const int wx = chunk * 64 + lane;
    const T* pl = ids + (long long)plane * hw;
    auto at = [&](int yy, int xx) -> int {
      if (yy < 0 || yy >= h || xx < 0 || xx >= w) return 0;
      EUNET_DASSERT(plane >= 0 && plane < p && (long long)yy * w + xx < hw);
      const long long v = (long long)pl[(long long)yy * w + xx];
      return v < 0 || v > t.n ? 0 : (int)v;
    };
    const int tr = at(wy - 1, wx), br = at(wy, wx);
    int tl = __shfl_up(tr, 1, 64), bl = __shfl_up(br, 1, 64);
    if (lane == 0) {
      tl = at(wy - 1, wx - 1);
      bl = at(wy, wx - 1);
    }
    // lanes past the last window of the row hold four zeros; a window of one label or of background adds nothing:
    // the area covers it
    const bool mixed = wx <= w && !(tl == tr && tr == bl && bl == br);
    const int v[4] = {tl, tr, bl, br};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int id = v[i];
      if (!mixed || id == 0) continue;
      unsigned mask = 0;
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (v[k] == id) mask |= 1u << k;
      if ((mask & ((1u << i) - 1u)) != 0) continue;  // counted at the label's first pixel of the window
      const int cnt = __popc(mask);
      const int col = cnt == 1 ? 10 : cnt == 3 ? 12 : (mask == 0x9u || mask == 0x6u) ? 13 : 11;
      const long long row = (long long)plane * (t.n + 1) + id;
      EUNET_DASSERT(cnt >= 1 && cnt <= 3 && id >= 1 && id <= t.n && row >= 1 && row < t.rows);
      add64(t.geom + row * GC + col, 1);
    }
  }
}

template <typename T>
void launch_cells(const void* ids, int p, int h, int w, const uint8_t* image, int c, const Tables& t,
                  int64_t* skipped, hipStream_t s) {
  const long long rows_px = (long long)p * h * ((w + WAVE_PX - 1) / WAVE_PX);
  const unsigned gm = grid_for(rows_px * 64, GRID_CAP);
  const T* src = (const T*)ids;
  long long* sk = (long long*)skipped;
  switch (c) {
    case 0:
      cell_init_kernel<0><<<grid_for(t.rows * GC, GRID_CAP), NT, 0, s>>>(t, h, w);
      cell_moments_kernel<T, 0><<<gm, NT, 0, s>>>(src, p, h, w, image, t, sk);
      break;
    case 1:
      cell_init_kernel<1><<<grid_for(t.rows * (GC + 4), GRID_CAP), NT, 0, s>>>(t, h, w);
      cell_moments_kernel<T, 1><<<gm, NT, 0, s>>>(src, p, h, w, image, t, sk);
      break;
    case 2:
      cell_init_kernel<2><<<grid_for(t.rows * (GC + 8), GRID_CAP), NT, 0, s>>>(t, h, w);
      cell_moments_kernel<T, 2><<<gm, NT, 0, s>>>(src, p, h, w, image, t, sk);
      break;
    default:
      cell_init_kernel<3><<<grid_for(t.rows * (GC + 12), GRID_CAP), NT, 0, s>>>(t, h, w);
      cell_moments_kernel<T, 3><<<gm, NT, 0, s>>>(src, p, h, w, image, t, sk);
      break;
  }
  const long long rows_win = (long long)p * (h + 1) * ((w + 1 + 63) / 64);
  cell_quads_kernel<T><<<grid_for(rows_win * 64, GRID_CAP), NT, 0, s>>>(src, p, h, w, t);
}

}  // namespace

extern "C" {

int eunet_cell_stats(const void* ids, int elem_bytes, int p, int h, int w, int n, const uint8_t* image, int c,
                     int64_t* geom, int64_t* inten, int64_t* skipped, void* stream) {
  EUNET_REQUIRE(ids && geom && skipped, "cell_stats: null pointer");
  EUNET_REQUIRE(elem_bytes == 4 || elem_bytes == 8, "cell_stats: int32 or int64 ids (elem_bytes 4 or 8)");
  EUNET_REQUIRE(plane_stack_ok(p, h, w, false),
                "cell_stats: bad shape (p 1..65535, h and w 1..%d)", EUNET_EDT_MAX_SIDE);
  EUNET_REQUIRE(n >= 0 && n <= EUNET_PAIRS_MAX_ID, "cell_stats: n must lie in 0..%d (got %d)", EUNET_PAIRS_MAX_ID, n);
  EUNET_REQUIRE(image ? (c >= 1 && c <= 3 && inten) : c == 0,
                "cell_stats: an image has 1..3 channels and an intensity table; without one c is 0");
  EUNET_REQUIRE(((uintptr_t)geom & 7u) == 0 && ((uintptr_t)skipped & 7u) == 0 && ((uintptr_t)inten & 7u) == 0 &&
                    ((uintptr_t)ids & (uintptr_t)(elem_bytes - 1)) == 0,
                "cell_stats: misaligned pointer");
  const hipStream_t s = (hipStream_t)stream;
  if (!fill_async(skipped, 0, sizeof(int64_t) * (size_t)p, s, "cell_stats")) return EUNET_ERR_HIP;
  const Tables t = {(long long*)geom, image ? (long long*)inten : nullptr, (long long)p * (n + 1), n};
  if (elem_bytes == 4) launch_cells<int32_t>(ids, p, h, w, image, c, t, skipped, s);
  else launch_cells<int64_t>(ids, p, h, w, image, c, t, skipped, s);
  EUNET_LAUNCH_CHECK("cell_stats");
  return EUNET_OK;
}

}  // extern "C"
