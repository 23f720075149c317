// Per-cell convex hulls: the hull of every label of a label map, its area, perimeter and the two Feret diameters as
// integers (eunet/metrics.py, hull_measurements).  The definitions are in include/eunet.h ("per-cell convex hulls").
//   hull_init_kernel     writes every output: the row extents of no pixel (w, -1), zero vertices, zero hull rows and
//                        the zero outside counts
//   hull_extents_kernel  one pass over the ids in cell_moments_kernel's wave layout (cellprops.hip): a wave holds 256
//                        consecutive pixels of one row, four per lane; the first pixel of every run of one measured id
//                        lowers the label's xmin of that row and raises its xmax with one 32-bit atomic each
//   hull_chain_kernel    one wave per label: the hull of the pixel squares is the hull of the corners of the row
//                        extents, which are sorted by y already, so Andrew's monotone chain needs no sort; lane 0 walks
//                        the rows (the other lanes load them, 64 levels at a time) with the label's own vertex slots
//                        as the stack, then the 64 lanes share the vertex-pair and the edge x vertex loops
// The caller's row layout (row_off, row_y0) is not trusted: a label whose slice does not lie inside 0..R is not
// measured and its pixels, like every measured pixel whose row falls outside its label's rows, are counted in
// outside[plane] and stored nowhere.  Every loop is bounded by the shapes, a label's rows or its vertex count; every
// result is an integer and independent of the order in which the atomics land.
#include "common.h"
#include "labelmap.h"

EUNET_DEBUG_UNIT(hull)

namespace {

constexpr int NT = 256;
static_assert(NT == LM_NT, "labelmap.h sizes blocks of NT");
constexpr int GRID_CAP = 4096;  // blocks of a grid-stride launch
constexpr int PV = 4;             // pixels a lane holds
constexpr int WAVE_PX = 64 * PV;  // pixels a wave holds
constexpr int HC = EUNET_CELL_HULL_COLS;
typedef unsigned long long u64;
typedef unsigned __int128 u128;

struct Layout {
  const long long* off;  // [L + 1], the first row of every label in ext; off[L] = R
  const int* y0;         // [L], the image row of a label's first row
  long long L;           // p (n + 1)
  int n;
};

// R as the kernels use it: a total outside 0..EUNET_CELL_HULL_MAX_ROWS admits no label at all
__device__ __forceinline__ long long total_rows(const Layout& t) {
  const long long R = t.off[t.L];
  return R < 0 || R > EUNET_CELL_HULL_MAX_ROWS ? 0 : R;
}

// the slice of label r: false where it does not lie inside 0..R in order (a layout that is not this map's)
__device__ __forceinline__ bool label_rows(const Layout& t, long long R, long long r, long long& base, long long& rows) {
  base = t.off[r];
  const long long end = t.off[r + 1];
  rows = end - base;
  return base >= 0 && rows >= 0 && rows <= EUNET_EDT_MAX_SIDE && end <= R;
}

__global__ __launch_bounds__(NT) void hull_init_kernel(Layout t, int p, int w, int* __restrict__ ext,
                                                       int* __restrict__ verts, long long* __restrict__ hull,
                                                       long long* __restrict__ outside) {
  const long long R = total_rows(t);
  const long long ne = 2 * R, nv = 4 * (R + t.L), nh = (long long)HC * t.L;
  const long long total = ne + nv + nh + p;
  for (long long i = (long long)blockIdx.x * NT + threadIdx.x; i < total; i += (long long)gridDim.x * NT) {
    if (i < ne) {
      ext[i] = (i & 1) ? -1 : w;
    } else if (i < ne + nv) {
      verts[i - ne] = 0;
    } else if (i < ne + nv + nh) {
      hull[i - ne - nv] = 0;
    } else {
      EUNET_DASSERT(i - ne - nv - nh >= 0 && i - ne - nv - nh < p);
      outside[i - ne - nv - nh] = 0;
    }
  }
}

// cell_moments_kernel's unit and run logic (cellprops.hip): grid-stride over units of WAVE_PX pixels, one per wave and
// round, unit = (plane, row, chunk of the row); whole waves only, lanes past the row's end hold key 0 and never write,
// and no lane leaves before the last shuffle.  The key of a pixel is its id when that lies in 1..n and 0 otherwise.  A
// boundary is a pixel whose key differs from the one before it in the chunk; a boundary with a measured id is a run
// head and issues the two atomics of its whole run, so a label's row costs two atomics per chunk it crosses.
template <typename T>
__global__ __launch_bounds__(NT) void hull_extents_kernel(const T* __restrict__ ids, int p, int h, int w, Layout t,
                                                          int* __restrict__ ext, long long* __restrict__ outside) {
  const int cpr = (w + WAVE_PX - 1) / WAVE_PX;  // chunks per row
  const long long units = (long long)p * h * cpr;
  const long long hw = (long long)h * w;
  const long long R = total_rows(t);
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
      for (int j = 0; j < PV; ++j) key[j] = v[j] < 0 || v[j] > t.n ? 0 : (int)v[j];
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
#pragma unroll
    for (int j = 0; j < PV; ++j) {
      if (!((bm >> j) & 1u) || key[j] == 0) continue;
      const unsigned rest = bm >> (j + 1);
      const int len = rest ? __ffs((int)rest) : PV - j + beyond;
      const int xa = x0 + j, xb = xa + len;  // the run is xa .. xb - 1
      EUNET_DASSERT(len >= 1 && lane * PV + j + len <= WAVE_PX && xb <= w && key[j] >= 1 && key[j] <= t.n);
      const long long r = (long long)plane * (t.n + 1) + key[j];
      EUNET_DASSERT(r >= 1 && r < t.L);
      long long first, rows;
      const bool ok = label_rows(t, R, r, first, rows);
      const long long yr = (long long)y - t.y0[r];
      if (ok && yr >= 0 && yr < rows) {
        EUNET_DASSERT(first + yr >= 0 && first + yr < R);
        int* e = ext + 2 * (first + yr);
        atomicMin(e, xa);
        atomicMax(e + 1, xb - 1);
      } else {
        EUNET_DASSERT(plane >= 0 && plane < p);
        atomicAdd((u64*)(outside + plane), (u64)len);
      }
    }
  }
}

// cross(b - a, c - a): positive where a -> b -> c turns the way the hull is listed (with y pointing down: top edge
// left to right, right chain downwards)
__device__ __forceinline__ long long cross3(int2 a, int2 b, int2 c) {
  return (long long)(b.x - a.x) * (c.y - a.y) - (long long)(b.y - a.y) * (c.x - a.x);
}

// The stack of the monotone chain in a label's vertex slots, kept by lane 0 alone: k entries, the top two also in
// registers (a below b), so that only a pop loads.
struct Stack {
  int2* v;
  int cap, k, high;  // high: the most entries the stack ever held
  int2 a, b;
  __device__ __forceinline__ void put(int2 q) {
    EUNET_DASSERT(k >= 0 && k < cap);
    if (k < cap) v[k] = q;
    ++k;
    high = k > high ? k : high;
    a = b;
    b = q;
  }
  // pops while the top turns the wrong way or not at all (collinear points go) and more than `keep` entries remain
  __device__ __forceinline__ void pop_for(int2 q, int keep) {
    while (k > keep && cross3(a, b, q) <= 0) {
      --k;
      b = a;
      EUNET_DASSERT(k < 2 || k - 2 < cap);
      if (k >= 2 && k - 2 < cap) a = v[k - 2];
    }
  }
};

// the corner points of level l of a label (the lattice row y0 + l, l = 0 .. rows) that can lie on the hull: the
// largest x + 1 and the smallest x over the rows l - 1 and l that hold a pixel; xr = 0 where neither does
__device__ __forceinline__ void level_points(const int2* __restrict__ e, long long rows, long long l, int& xr, int& xl) {
  int lo = 0x7fffffff, hi = -1;
#pragma unroll
  for (int d = -1; d <= 0; ++d) {
    const long long row = l + d;
    if (row < 0 || row >= rows) continue;
    const int2 q = e[row];
    if (q.y >= q.x) {
      lo = q.x < lo ? q.x : lo;
      hi = q.y > hi ? q.y : hi;
    }
  }
  xr = hi + 1;
  xl = lo;
}

// floor(2^16 sqrt(d2)) with the correctly rounded fp64 root of the exact integer (d2 <= 2^27: the product is exact)
__device__ __forceinline__ long long q16_length(long long d2) { return (long long)(65536.0 * sqrt((double)d2)); }

struct Width {  // the candidate of the minimum width: c over the edge (dx, dy) of index k; k < 0: none
  int c, dx, dy, k;
};
// a before b in the order (c^2 / |e|^2, k): the products reach 2^81
__device__ __forceinline__ bool narrower(const Width& a, const Width& b) {
  if (a.k < 0 || b.k < 0) return b.k < 0 && a.k >= 0;
  const u128 la = (u128)((u64)a.c * (u64)a.c) * (u64)((long long)b.dx * b.dx + (long long)b.dy * b.dy);
  const u128 lb = (u128)((u64)b.c * (u64)b.c) * (u64)((long long)a.dx * a.dx + (long long)a.dy * a.dy);
  return la < lb || (la == lb && a.k < b.k);
}

// grid-stride over the labels, one per wave and round; whole waves only (the shuffles need every lane)
__global__ __launch_bounds__(NT) void hull_chain_kernel(Layout t, const int* __restrict__ ext, int* verts,
                                                        long long* __restrict__ hull) {
  const long long R = total_rows(t);
  const int lane = threadIdx.x & 63;
  const long long wave = (long long)blockIdx.x * (NT / 64) + (threadIdx.x >> 6);
  const long long waves = (long long)gridDim.x * (NT / 64);
  for (long long r = wave; r < t.L; r += waves) {
    long long first, rows;
    if (r % (t.n + 1) == 0 || !label_rows(t, R, r, first, rows) || rows == 0) continue;  // the same for the wave
    EUNET_DASSERT(first >= 0 && first + rows <= R && 2 * (first + r) + 2 * (rows + 1) <= 2 * (R + t.L));
    const int2* e = reinterpret_cast<const int2*>(ext) + first;
    int2* V = reinterpret_cast<int2*>(verts) + 2 * (first + r);
    const int y0 = t.y0[r];
    Stack s = {V, (int)(2 * (rows + 1)), 0, 0, make_int2(0, 0), make_int2(0, 0)};
    int2 tl = make_int2(0, 0);
    long long lf = -1;  // the first level with a point
    // the chain from the top left corner along the top edge and down the right side to the bottom right corner
    for (long long l0 = 0; l0 <= rows; l0 += 64) {
      int XR = 0, XL = 0;
      if (l0 + lane <= rows) level_points(e, rows, l0 + lane, XR, XL);
      const int cnt = (int)(rows + 1 - l0 < 64 ? rows + 1 - l0 : 64);
      for (int j = 0; j < cnt; ++j) {
        const int xr = __shfl(XR, j, 64), xl = __shfl(XL, j, 64);
        if (lane != 0 || xr <= 0) continue;
        const int2 q = make_int2(xr, y0 + (int)(l0 + j));
        if (s.k == 0) {
          lf = l0 + j;
          tl = make_int2(xl, q.y);
          s.put(tl);
        } else {
          s.pop_for(q, 2);
        }
        s.put(q);
      }
    }
    // and back: along the bottom edge and up the left side; the bottom right corner stays, the top left corner ends
    // the chain without being listed twice
    const int na = s.k;
    bool done = na == 0;
    for (long long l0 = rows / 64 * 64; l0 >= 0; l0 -= 64) {
      int XR = 0, XL = 0;
      if (l0 + lane <= rows) level_points(e, rows, l0 + lane, XR, XL);
      const int cnt = (int)(rows + 1 - l0 < 64 ? rows + 1 - l0 : 64);
      for (int j = cnt - 1; j >= 0; --j) {
        const int xr = __shfl(XR, j, 64), xl = __shfl(XL, j, 64);
        if (lane != 0 || xr <= 0 || done) continue;
        const int2 q = make_int2(xl, y0 + (int)(l0 + j));
        s.pop_for(q, na);
        if (l0 + j == lf) done = true;
        else s.put(q);
      }
    }
    if (lane == 0) {
      EUNET_DASSERT(s.k <= s.cap && (s.k == 0 || s.k >= 4));
      const int top = s.high < s.cap ? s.high : s.cap;
      for (int i = s.k; i < top; ++i) V[i] = make_int2(0, 0);  // what the stack held past the hull
    }
    const int nv = __shfl(s.k < s.cap ? s.k : s.cap, 0, 64);
    if (nv == 0) continue;  // rows without a pixel: the row of zeros stays
    __threadfence();        // lane 0's vertices, for the other lanes' loads

    // the largest squared distance of two vertices, the smallest (i, j) first among equals: one key to maximise
    u64 far = 0;
    for (int i = lane; i < nv; i += 64) {
      const int2 a = V[i];
      for (int j = i + 1; j < nv; ++j) {
        const int2 b = V[j];
        const u64 d2 = (u64)((long long)(b.x - a.x) * (b.x - a.x) + (long long)(b.y - a.y) * (b.y - a.y));
        const u64 key = d2 << 32 | (u64)(0xffff - i) << 16 | (u64)(0xffff - j);
        far = key > far ? key : far;
      }
    }
    // per edge: the shoelace term, the length and the farthest vertex from its line
    long long area2 = 0, length = 0;
    Width best = {0, 0, 0, -1};
    for (int k = lane; k < nv; k += 64) {
      const int2 a = V[k], b = V[k + 1 < nv ? k + 1 : 0];
      const int dx = b.x - a.x, dy = b.y - a.y;
      area2 += (long long)a.x * b.y - (long long)b.x * a.y;
      length += q16_length((long long)dx * dx + (long long)dy * dy);
      long long c = 0;
      for (int i = 0; i < nv; ++i) {
        const long long v = cross3(a, b, V[i]);
        c = v > c ? v : c;
      }
      const Width cand = {(int)c, dx, dy, k};
      if (narrower(cand, best)) best = cand;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const u64 f = __shfl_xor(far, o, 64);
      far = f > far ? f : far;
      area2 += __shfl_xor(area2, o, 64);
      length += __shfl_xor(length, o, 64);
      const Width other = {__shfl_xor(best.c, o, 64), __shfl_xor(best.dx, o, 64), __shfl_xor(best.dy, o, 64),
                           __shfl_xor(best.k, o, 64)};
      if (narrower(other, best)) best = other;
    }
    if (lane == 0) {
      const int i = 0xffff - (int)((far >> 16) & 0xffff), j = 0xffff - (int)(far & 0xffff);
      EUNET_DASSERT(i >= 0 && i < j && j < nv && best.k >= 0 && best.k < nv && r >= 1 && r < t.L);
      const int2 a = V[i < nv ? i : 0], b = V[j < nv ? j : 0];
      long long* row = hull + r * HC;
      row[0] = nv;
      row[1] = area2;
      row[2] = length;
      row[3] = (long long)(far >> 32);
      row[4] = a.x;
      row[5] = a.y;
      row[6] = b.x;
      row[7] = b.y;
      row[8] = best.c;
      row[9] = best.dx;
      row[10] = best.dy;
    }
  }
}

}  // namespace

extern "C" {

int eunet_cell_hulls(const void* ids, int elem_bytes, int p, int h, int w, int n, const int64_t* row_off,
                     const int32_t* row_y0, int32_t* ext, int32_t* verts, int64_t* hull, int64_t* outside,
                     void* stream) {
  EUNET_REQUIRE(ids && row_off && row_y0 && ext && verts && hull && outside, "cell_hulls: null pointer");
  EUNET_REQUIRE(elem_bytes == 4 || elem_bytes == 8, "cell_hulls: int32 or int64 ids (elem_bytes 4 or 8)");
  EUNET_REQUIRE(plane_stack_ok(p, h, w, false),
                "cell_hulls: bad shape (p 1..65535, h and w 1..%d)", EUNET_EDT_MAX_SIDE);
  EUNET_REQUIRE(n >= 0 && n <= EUNET_PAIRS_MAX_ID, "cell_hulls: n must lie in 0..%d (got %d)", EUNET_PAIRS_MAX_ID, n);
  EUNET_REQUIRE(((uintptr_t)row_off & 7u) == 0 && ((uintptr_t)row_y0 & 3u) == 0 && ((uintptr_t)ext & 7u) == 0 &&
                    ((uintptr_t)verts & 7u) == 0 && ((uintptr_t)hull & 7u) == 0 && ((uintptr_t)outside & 7u) == 0 &&
                    ((uintptr_t)ids & (uintptr_t)(elem_bytes - 1)) == 0,
                "cell_hulls: misaligned pointer");
  const hipStream_t s = (hipStream_t)stream;
  const Layout t = {(const long long*)row_off, row_y0, (long long)p * (n + 1), n};
  // R is on the device only; a label has at most h rows
  const long long most = t.L * (6ll * h + 4 + HC) + p;
  hull_init_kernel<<<grid_for(most, GRID_CAP), NT, 0, s>>>(t, p, w, ext, verts, (long long*)hull, (long long*)outside);
  const unsigned ge = grid_for((long long)p * h * ((w + WAVE_PX - 1) / WAVE_PX) * 64, GRID_CAP);
  if (elem_bytes == 4)
    hull_extents_kernel<int32_t><<<ge, NT, 0, s>>>((const int32_t*)ids, p, h, w, t, ext, (long long*)outside);
  else
    hull_extents_kernel<int64_t><<<ge, NT, 0, s>>>((const int64_t*)ids, p, h, w, t, ext, (long long*)outside);
  hull_chain_kernel<<<grid_for(t.L * 64, GRID_CAP), NT, 0, s>>>(t, ext, verts, (long long*)hull);
  EUNET_LAUNCH_CHECK("cell_hulls");
  return EUNET_OK;
}

}  // extern "C"
