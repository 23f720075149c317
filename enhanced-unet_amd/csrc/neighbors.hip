// Cells in relation to each other: the nearest-cell (feature) transform, label expansion and the contact table.
//
// No reference line: the reference counts cells and relates none to another.  The definitions are in include/eunet.h
// ("nearest-cell transform, label expansion and cell contacts"): the sites of a plane are its pixels with id >= 1, and
// (dist, site) of a pixel is the lexicographic minimum of (squared distance, linear index) over the sites.
//   site_cols_kernel   one thread per column, siblings of boundary.hip's column sweeps: a down sweep leaves the row of
//                      the nearest site at or above, an up sweep combines it with the nearest below (the smaller row
//                      of two equally near) and leaves the ROW of the column's nearest site, -1 without one
//   site_rows_kernel   one block per row: that row of site rows staged whole in LDS (so the pass runs in place), g =
//                      (y - row)^2 formed on the fly; each pixel scans outward from r = 0, keeps the smallest
//                      (g + r^2) << 32 | index and stops at the first r with r^2 > best, strictly: at r^2 == best a
//                      site of the pixel's own row ties the best and may have the smaller index.  EXPAND: the
//                      pixel's id is gathered from the winner instead of storing (dist, site); pixels that carry an id
//                      scan nothing, and a limited expansion scans no further than r^2 <= limit2
//   contacts_kernel    one pass; a wave holds 256 consecutive pixels of one row, four per lane, with the row below;
//                      each direction's keys (plane, min id, max id) are collapsed into runs along the row as
//                      pairs.hip's, a run head inserts (key, run length) into labelmap.h's table
// Every loop is bounded by h, w or the probe count, no block waits on another, every result is an integer and
// independent of the order in which the atomics land.
#include "common.h"
#include "labelmap.h"

EUNET_DEBUG_UNIT(neighbors)

namespace {

constexpr int COL_NT = 64;  // a wave per block, as boundary.hip's column pass: 1024 columns still spread over 16 CUs
constexpr int COL_CH = 16;  // rows per chunk of the column sweeps
constexpr int ROW_NT = 256;
constexpr int NT = 256;
static_assert(NT == LM_NT, "labelmap.h sizes blocks of NT");
constexpr int GRID_CAP = 2048;    // blocks of a grid-stride launch
constexpr int PV = 4;             // pixels a lane holds
constexpr int WAVE_PX = 64 * PV;  // pixels of a row a wave holds
constexpr long long ID_MAX = EUNET_PAIRS_MAX_ID;
constexpr unsigned NONE = (unsigned)EUNET_EDT_NONE;
constexpr unsigned long long NO_SITE = ~0ull;

// grid (ceil(w / COL_NT), p): thread = one column of one plane.  Both sweeps go in chunks of COL_CH rows: a chunk's
// loads are issued together (from a clamped row, so none is conditional), then the recurrence runs in registers.
template <typename T>
__global__ __launch_bounds__(COL_NT) void site_cols_kernel(const T* __restrict__ ids, int h, int w,
                                                           int32_t* __restrict__ rows) {
  const int x = blockIdx.x * COL_NT + (int)threadIdx.x;
  if (x >= w) return;  // no shuffle and no barrier below
  const long long hw = (long long)h * w;
  const T* src = ids + (long long)blockIdx.y * hw + x;
  int32_t* o = rows + (long long)blockIdx.y * hw + x;

  int up = -1;  // the last site row at or above
  for (int y0 = 0; y0 < h; y0 += COL_CH) {
    unsigned sites = 0u;  // bit i: (y0 + i, x) is a site
#pragma unroll
    for (int i = 0; i < COL_CH; ++i) {
      const int y = y0 + i < h ? y0 + i : h - 1;
      sites |= (unsigned)((long long)src[(long long)y * w] >= 1) << i;
    }
#pragma unroll
    for (int i = 0; i < COL_CH; ++i) {
      const int y = y0 + i;
      if (y < h) {
        up = ((sites >> i) & 1u) ? y : up;
        o[(long long)y * w] = up;
      }
    }
  }
  int dn = -1;  // the last site row at or below
  for (int y1 = h; y1 > 0; y1 -= COL_CH) {  // the rows y1 - 1 down to y1 - COL_CH
    int t[COL_CH];
#pragma unroll
    for (int i = 0; i < COL_CH; ++i) {
      const int y = y1 - 1 - i;
      t[i] = o[(long long)(y < 0 ? 0 : y) * w];
    }
#pragma unroll
    for (int i = 0; i < COL_CH; ++i) {
      const int y = y1 - 1 - i;
      if (y >= 0) {
        const int u = t[i];
        EUNET_DASSERT(u >= -1 && u <= y);
        dn = u == y ? y : dn;
        // equally near above and below: the row above has the smaller index
        o[(long long)y * w] = (u >= 0 && (dn < 0 || y - u <= dn - y)) ? u : dn;
      }
    }
  }
}

// grid (h, p): block = one row of one plane.  rows: the column pass's output, [p][h][w]; without EXPAND it is also
// where the site indices go (in place: a block reads its row into LDS before it writes it, and touches no other).
// (g + r^2) <= 2 * 8191^2 < 2^31 and index < 2^26: the pair packs into 64 bits whose order is the lexicographic one.
template <typename T, bool EXPAND>
__global__ __launch_bounds__(ROW_NT) void site_rows_kernel(int32_t* rows, int32_t* __restrict__ dist,
                                                           const T* __restrict__ ids, T* __restrict__ out, int w,
                                                           long long limit2) {
  extern __shared__ __attribute__((aligned(16))) int srow[];
  const int y = blockIdx.x, h = gridDim.x;
  const long long pbase = (long long)blockIdx.y * h * w;  // of the plane
  const long long base = pbase + (long long)y * w;        // of the row
  int any = 0;
  for (int x = threadIdx.x; x < w; x += ROW_NT) {
    const int t = rows[base + x];
    EUNET_DASSERT(t >= -1 && t < h);
    srow[x] = t;
    any |= t >= 0;
  }
  if (!__syncthreads_or(any)) {  // no site in the plane: every row is such a row
    for (int x = threadIdx.x; x < w; x += ROW_NT) {
      if (EXPAND) {
        out[base + x] = ids[base + x];
      } else {
        dist[base + x] = (int32_t)NONE;
        rows[base + x] = -1;
      }
    }
    return;
  }
  // r^2 beyond which nothing is looked at: none for the transform and the unlimited expansion
  const unsigned stop2 = EXPAND && limit2 >= 0 && limit2 < (long long)NONE ? (unsigned)limit2 : NONE;
  for (int x = threadIdx.x; x < w; x += ROW_NT) {
    if (EXPAND) {
      const T v = ids[base + x];
      if (v != 0) {  // a label or an ignored pixel keeps its id
        out[base + x] = v;
        continue;
      }
    }
    auto cand = [&](int xx, unsigned r2) -> unsigned long long {
      EUNET_DASSERT(xx >= 0 && xx < w);
      const int row = srow[xx];
      const unsigned dy = (unsigned)(row > y ? row - y : y - row);
      const unsigned long long key =
          ((unsigned long long)(dy * dy + r2) << 32) | (unsigned long long)(unsigned)(row * w + xx);
      return row < 0 ? NO_SITE : key;
    };
    unsigned long long best = cand(x, 0u);
    const int reach = x > w - 1 - x ? x : w - 1 - x;
    for (int r = 1; r <= reach; ++r) {
      const unsigned r2 = (unsigned)r * (unsigned)r;
      if (r2 > (unsigned)(best >> 32) || r2 > stop2) break;  // NO_SITE >> 32 is above every r^2
      if (x - r >= 0) {
        const unsigned long long c = cand(x - r, r2);
        best = c < best ? c : best;
      }
      if (x + r < w) {
        const unsigned long long c = cand(x + r, r2);
        best = c < best ? c : best;
      }
    }
    EUNET_DASSERT(EXPAND || best != NO_SITE);  // a full scan meets the row's site
    const unsigned d2 = best == NO_SITE ? NONE : (unsigned)(best >> 32);
    const int idx = best == NO_SITE ? -1 : (int)(unsigned)(best & 0xffffffffull);
    EUNET_DASSERT(idx >= -1 && (long long)idx < (long long)h * w);
    if (EXPAND) {
      const bool take = idx >= 0 && (limit2 < 0 || (long long)d2 <= limit2);
      out[base + x] = take ? ids[pbase + idx] : (T)0;
    } else {
      dist[base + x] = (int32_t)d2;
      rows[base + x] = idx;
    }
  }
}

// ---- contacts ------------------------------------------------------------------------------------------------
// an id as the contact pass sees it: 1..ID_MAX itself, everything else 0 ("takes no part"); *over: it was above ID_MAX
__device__ __forceinline__ int contact_id(long long v, bool* over) {
  *over = v > ID_MAX;
  return v >= 1 && v <= ID_MAX ? (int)v : 0;
}

// the PV ids of the columns x0 .. x0 + PV - 1 of a row (null: a row outside the plane), 0 past the row's end.  VEC:
// every row starts on a 16-byte boundary and w is a multiple of PV, so a lane inside the row reads 16 bytes at a time.
template <typename T, bool VEC>
__device__ __forceinline__ void load_row(const T* __restrict__ row, int x0, int w, int (&v)[PV], unsigned* bad) {
  long long t[PV] = {0, 0, 0, 0};
  if (row && x0 < w) {
    if (VEC) {
      EUNET_DASSERT(x0 + PV <= w);
      if constexpr (sizeof(T) == 4) {
        const int4 q = *reinterpret_cast<const int4*>(row + x0);
        t[0] = q.x; t[1] = q.y; t[2] = q.z; t[3] = q.w;
      } else {
        const longlong2 q0 = *reinterpret_cast<const longlong2*>(row + x0);
        const longlong2 q1 = *reinterpret_cast<const longlong2*>(row + x0 + 2);
        t[0] = q0.x; t[1] = q0.y; t[2] = q1.x; t[3] = q1.y;
      }
    } else {
#pragma unroll
      for (int j = 0; j < PV; ++j) t[j] = x0 + j < w ? (long long)row[x0 + j] : 0ll;
    }
  }
#pragma unroll
  for (int j = 0; j < PV; ++j) {
    bool over;
    v[j] = contact_id(t[j], &over);
    *bad += over;
  }
}

// one id of a row, 0 outside it
template <typename T>
__device__ __forceinline__ int load_one(const T* __restrict__ row, int x, int w) {
  bool over;
  return row && x >= 0 && x < w ? contact_id((long long)row[x], &over) : 0;
}

__device__ __forceinline__ unsigned long long contact_key(unsigned long long plane, int a, int b) {
  const int lo = a < b ? a : b, hi = a < b ? b : a;
  return lo > 0 && lo != hi ? (plane << 48) | ((unsigned long long)lo << 24) | (unsigned long long)hi : EMPTY;
}

// The wave's WAVE_PX keys of one direction, PV per lane in row order: a boundary is a key that differs from the one
// before it (the first is one); a boundary with a key other than EMPTY is a run head and inserts (key, run length),
// its run ending at the next boundary or with the wave.  Every lane of the wave calls it.
__device__ __forceinline__ void add_runs(const Table& t, const unsigned long long (&key)[PV], int lane) {
  unsigned long long prev = __shfl_up(key[PV - 1], 1, 64);
  unsigned bm = 0;  // bit j: key j of this lane is a boundary
#pragma unroll
  for (int j = 0; j < PV; ++j) {
    if ((j == 0 && lane == 0) || key[j] != prev) bm |= 1u << j;
    prev = key[j];
  }
  // the first boundary after this lane's keys: in lane nl, at its key ctz(nbm)
  const unsigned long long anyb = __ballot(bm != 0);
  const unsigned long long above = lane == 63 ? 0ull : anyb >> (lane + 1);
  const int nl = above ? lane + __ffsll((long long)above) : lane;
  const unsigned nbm = __shfl(bm, nl, 64);
  const int beyond = above ? PV * (nl - lane - 1) + (__ffs((int)nbm) - 1) : PV * (63 - lane);
#pragma unroll
  for (int j = 0; j < PV; ++j) {
    if (!((bm >> j) & 1u) || key[j] == EMPTY) continue;
    const unsigned rest = bm >> (j + 1);
    const int len = rest ? __ffs((int)rest) : PV - j + beyond;
    EUNET_DASSERT(len >= 1 && lane * PV + j + len <= WAVE_PX);
    table_update<TableAdd>(t, key[j], len);
  }
}

// grid-stride over units of WAVE_PX pixels of one row, one unit per wave and round; whole waves only (the shuffles
// and ballots need every lane: a lane past the row's end holds ids 0).  cur[j] is the pixel x0 + j (cur[PV]: the
// first of the next lane), low[k] the pixel x0 - 1 + k of the row below; the ends of the wave read theirs from memory.
template <typename T, bool VEC, bool CONN8>
__global__ __launch_bounds__(NT) void contacts_kernel(const T* __restrict__ ids, int p, int h, int w, Table t,
                                                      unsigned long long* invalid) {
  const int segs = (w + WAVE_PX - 1) / WAVE_PX;
  const long long units = (long long)p * h * segs;
  const int lane = threadIdx.x & 63;
  const long long wave = (long long)blockIdx.x * (NT / 64) + (threadIdx.x >> 6);
  const long long waves = (long long)gridDim.x * (NT / 64);
  unsigned bad = 0;
  for (long long u = wave; u < units; u += waves) {
    const int seg = (int)(u % segs);
    const long long py = u / segs;
    const int y = (int)(py % h);
    const long long plane = py / h;
    EUNET_DASSERT(plane >= 0 && plane < p && y >= 0 && y < h);
    const int x0 = seg * WAVE_PX + lane * PV;
    const T* row = ids + (plane * h + y) * (long long)w;
    const T* below = y + 1 < h ? row + w : nullptr;
    int cur[PV + 1], low[PV + 2];
    unsigned nobad = 0;  // the row below is counted when it is the wave's own
    {
      int c[PV], l[PV];
      load_row<T, VEC>(row, x0, w, c, &bad);
      load_row<T, VEC>(below, x0, w, l, &nobad);
#pragma unroll
      for (int j = 0; j < PV; ++j) {
        cur[j] = c[j];
        low[j + 1] = l[j];
      }
    }
    cur[PV] = __shfl_down(cur[0], 1, 64);
    low[PV + 1] = __shfl_down(low[1], 1, 64);
    low[0] = __shfl_up(low[PV], 1, 64);
    if (lane == 63) {
      cur[PV] = load_one(row, x0 + PV, w);
      low[PV + 1] = load_one(below, x0 + PV, w);
    }
    if (lane == 0) low[0] = load_one(below, x0 - 1, w);

    unsigned long long key[CONN8 ? 4 : 2][PV];
    bool some = false;
#pragma unroll
    for (int j = 0; j < PV; ++j) {
      key[0][j] = contact_key((unsigned long long)plane, cur[j], cur[j + 1]);  // right
      key[1][j] = contact_key((unsigned long long)plane, cur[j], low[j + 1]);  // down
      some |= key[0][j] != EMPTY || key[1][j] != EMPTY;
      if (CONN8) {
        key[2][j] = contact_key((unsigned long long)plane, cur[j], low[j]);      // down left
        key[3][j] = contact_key((unsigned long long)plane, cur[j], low[j + 2]);  // down right
        some |= key[2][j] != EMPTY || key[3][j] != EMPTY;
      }
    }
    if (!__ballot(some)) continue;  // the same in every lane: only a wave on a border inserts
#pragma unroll
    for (int d = 0; d < (CONN8 ? 4 : 2); ++d) add_runs(t, key[d], lane);
  }
  bad = wave_sum(bad);
  if (lane == 0 && bad) atomicAdd(invalid, (unsigned long long)bad);
}

bool ids_ok(const void* ids, int elem_bytes) {
  return ids && (elem_bytes == 4 || elem_bytes == 8) && ((uintptr_t)ids & (uintptr_t)(elem_bytes - 1)) == 0;
}

template <typename T>
void launch_cols(const void* ids, int p, int h, int w, int32_t* rows, hipStream_t s) {
  site_cols_kernel<T><<<dim3((unsigned)cdiv(w, COL_NT), (unsigned)p), COL_NT, 0, s>>>((const T*)ids, h, w, rows);
}

template <typename T>
void launch_contacts(const void* ids, int p, int h, int w, bool conn8, const Table& t, int64_t* invalid,
                     hipStream_t s) {
  const long long units = (long long)p * h * cdiv(w, WAVE_PX);
  const unsigned g = grid_for(units * 64, GRID_CAP);
  const bool vec = w % PV == 0 && ((uintptr_t)ids & 15u) == 0;
  by_flag(vec, [&](auto v) {
    by_flag(conn8, [&](auto c) {
      contacts_kernel<T, decltype(v)::value, decltype(c)::value>
          <<<g, NT, 0, s>>>((const T*)ids, p, h, w, t, (unsigned long long*)invalid);
    });
  });
}

}  // namespace

extern "C" {

int eunet_nearest_site(const void* ids, int elem_bytes, int p, int h, int w, int32_t* dist, int32_t* site,
                       void* stream) {
  EUNET_REQUIRE(ids_ok(ids, elem_bytes) && dist && site, "nearest_site: null or misaligned ids (int32 or int64), or "
                "null outputs");
  EUNET_REQUIRE(plane_stack_ok(p, h, w, false), "nearest_site: bad shape (p 1..65535, h and w 1..%d)",
                EUNET_EDT_MAX_SIDE);
  EUNET_REQUIRE((((uintptr_t)dist | (uintptr_t)site) & 3u) == 0, "nearest_site: misaligned dist / site");
  const hipStream_t s = (hipStream_t)stream;
  const dim3 gr((unsigned)h, (unsigned)p);
  if (elem_bytes == 4) {
    launch_cols<int32_t>(ids, p, h, w, site, s);
    site_rows_kernel<int32_t, false><<<gr, ROW_NT, (size_t)w * 4, s>>>(site, dist, nullptr, nullptr, w, -1);
  } else {
    launch_cols<int64_t>(ids, p, h, w, site, s);
    site_rows_kernel<int64_t, false><<<gr, ROW_NT, (size_t)w * 4, s>>>(site, dist, nullptr, nullptr, w, -1);
  }
  EUNET_LAUNCH_CHECK("nearest_site");
  return EUNET_OK;
}

int eunet_expand_label_map(const void* ids, int elem_bytes, int p, int h, int w, long long limit2, int32_t* ws,
                           void* out, void* stream) {
  EUNET_REQUIRE(ids_ok(ids, elem_bytes) && ids_ok(out, elem_bytes) && ws,
                "expand_label_map: null or misaligned ids / out (int32 or int64), or null workspace");
  EUNET_REQUIRE(plane_stack_ok(p, h, w, false), "expand_label_map: bad shape (p 1..65535, h and w 1..%d)",
                EUNET_EDT_MAX_SIDE);
  EUNET_REQUIRE(((uintptr_t)ws & 3u) == 0, "expand_label_map: misaligned workspace");
  const size_t bytes = (size_t)p * h * w * (size_t)elem_bytes;
  EUNET_REQUIRE((const char*)out + bytes <= (const char*)ids || (const char*)ids + bytes <= (const char*)out,
                "expand_label_map: out overlaps ids");
  const hipStream_t s = (hipStream_t)stream;
  const dim3 gr((unsigned)h, (unsigned)p);
  if (elem_bytes == 4) {
    launch_cols<int32_t>(ids, p, h, w, ws, s);
    site_rows_kernel<int32_t, true>
        <<<gr, ROW_NT, (size_t)w * 4, s>>>(ws, nullptr, (const int32_t*)ids, (int32_t*)out, w, limit2);
  } else {
    launch_cols<int64_t>(ids, p, h, w, ws, s);
    site_rows_kernel<int64_t, true>
        <<<gr, ROW_NT, (size_t)w * 4, s>>>(ws, nullptr, (const int64_t*)ids, (int64_t*)out, w, limit2);
  }
  EUNET_LAUNCH_CHECK("expand_label_map");
  return EUNET_OK;
}

int eunet_label_contacts(const void* ids, int elem_bytes, int p, int h, int w, int connectivity, int64_t* keys,
                         int32_t* counts, long long capacity, int32_t* overflow, int64_t* invalid, void* stream) {
  EUNET_REQUIRE(ids_ok(ids, elem_bytes) && keys && counts && overflow && invalid,
                "label_contacts: null or misaligned ids (int32 or int64), or null table");
  EUNET_REQUIRE(plane_stack_ok(p, h, w, false), "label_contacts: bad shape (p 1..65535, h and w 1..%d)",
                EUNET_EDT_MAX_SIDE);
  EUNET_REQUIRE(connectivity == 4 || connectivity == 8, "label_contacts: connectivity 4 or 8 (got %d)", connectivity);
  EUNET_REQUIRE(((uintptr_t)keys & 7u) == 0 && ((uintptr_t)invalid & 7u) == 0, "label_contacts: misaligned pointer");
  const hipStream_t s = (hipStream_t)stream;
  Table t;
  const int rc = table_init("label_contacts", keys, counts, capacity, overflow, s, &t);
  if (rc != EUNET_OK) return rc;
  if (!fill_async(invalid, 0, sizeof(int64_t), s, "label_contacts")) return EUNET_ERR_HIP;
  if (elem_bytes == 4) launch_contacts<int32_t>(ids, p, h, w, connectivity == 8, t, invalid, s);
  else launch_contacts<int64_t>(ids, p, h, w, connectivity == 8, t, invalid, s);
  EUNET_LAUNCH_CHECK("label_contacts");
  return EUNET_OK;
}

}  // extern "C"
