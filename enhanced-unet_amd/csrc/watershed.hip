// Distance-transform watershed: the basins of a squared-distance map and the saddles between them.
//
// Reference: train_eval.py:654-850 (semantic_to_instances promises "使用分水岭算法进一步分离" and imports
// peak_local_max, but runs a ladder of fixed erosions).  This is the split the docstring names, in a form that is
// integer and order-free (the definition is in include/eunet.h, "distance-transform watershed"):
//   ws_up_kernel       one wave per strip of 62 columns: three rows of D live in registers, the horizontal
//                      neighbours come from the neighbouring lanes; parent = the 3x3 neighbour of largest key
//   ws_jump_kernel     pointer jumping, in place, a fixed number of launches that stop working once a round
//                      changed nothing (a device flag per round, no host read)
//   ws_first_kernel    the raster-first pixel of every basin (atomicMin, one per run of a basin in a wave)
//   ws_count / scan_block_counts (labelmap.h) / ws_rank / ws_fill   basins numbered 1..nb per plane in raster order
//                      of their first pixel
//   ws_peaks_kernel    root and peak of every basin, for the host's merge
//   ws_saddles_kernel  max over the 8-adjacent pixel pairs of two basins of min(D, D), into an open-addressing hash
//                      table keyed by the pair (atomicCAS insert, atomicMax value); equal pairs of a wave go in once
//   ws_relabel_kernel  basin -> final id through the host's merged table, and the areas
// The merge itself runs on the host over the basin graph (eunet/ops.py, merge_basins).
// Every loop is bounded by the shapes or by a constant, no block waits on another, every result is an integer and
// independent of the order in which the atomics land.
#include "common.h"
#include "labelmap.h"

EUNET_DEBUG_UNIT(watershed)

namespace {

constexpr int NT = 256;
static_assert(NT == LM_NT, "labelmap.h sizes and scans blocks of NT");
constexpr int GRID_CAP = 2048;      // blocks along x of a grid-stride launch
constexpr int UP_NT = 64;           // a wave per block
constexpr int UP_W = UP_NT - 2;     // columns a wave writes: its first and last lane hold the neighbouring columns
constexpr int UP_ROWS = 32;         // rows a wave walks down
constexpr int MIN_MATES = 4;        // lanes that must share a pair before the wave combines them

// grid (ceil(w / UP_W), ceil(h / UP_ROWS), p).  key(q) = (D[q], -q): a candidate replaces the best so far only when
// its D is strictly larger, and the candidates are visited in ascending linear index, so the smallest index among
// the largest D wins.  Background and positions outside the image read as 0 and can never beat the centre (D > 0).
__global__ __launch_bounds__(UP_NT) void ws_up_kernel(const int32_t* __restrict__ dist, int h, int w,
                                                      int32_t* __restrict__ parent) {
  const int lane = threadIdx.x;
  const int x = blockIdx.x * UP_W + lane - 1;  // -1 and w read as background
  const bool inx = x >= 0 && x < w;
  const bool writer = lane >= 1 && lane <= UP_W && x < w;  // no early return: the shuffles need the wave
  const long long hw = (long long)h * w;
  const int32_t* d = dist + (long long)blockIdx.z * hw;
  int32_t* par = parent + (long long)blockIdx.z * hw;
  const int y0 = blockIdx.y * UP_ROWS;
  const int y1 = y0 + UP_ROWS < h ? y0 + UP_ROWS : h;
  auto load = [&](int y) -> int { return (inx && y >= 0 && y < h) ? d[(long long)y * w + x] : 0; };
  int aC = load(y0 - 1), cC = load(y0);
  int aL = __shfl_up(aC, 1, 64), aR = __shfl_down(aC, 1, 64);
  int cL = __shfl_up(cC, 1, 64), cR = __shfl_down(cC, 1, 64);
  for (int y = y0; y < y1; ++y) {
    const int bC = load(y + 1);
    const int bL = __shfl_up(bC, 1, 64), bR = __shfl_down(bC, 1, 64);
    if (writer) {
      const int i = y * w + x;  // h * w < 2^31
      int up = -1;
      if (cC > 0) {
        int best = 0;
        if (aL > best) { best = aL; up = i - w - 1; }
        if (aC > best) { best = aC; up = i - w; }
        if (aR > best) { best = aR; up = i - w + 1; }
        if (cL > best) { best = cL; up = i - 1; }
        if (cC > best) { best = cC; up = i; }
        if (cR > best) { best = cR; up = i + 1; }
        if (bL > best) { best = bL; up = i + w - 1; }
        if (bC > best) { best = bC; up = i + w; }
        if (bR > best) { best = bR; up = i + w + 1; }
        EUNET_DASSERT(up >= 0 && (long long)up < hw);
      }
      EUNET_DASSERT(i >= 0 && (long long)i < hw);
      par[i] = up;
    }
    aL = cL; aC = cC; aR = cR;
    cL = bL; cC = bC; cR = bR;
  }
}

// grid (gx, p).  root[i] <- root[root[i]], in place.  Safe without a second buffer: every value ever stored in
// root[a] is an ancestor of a (its parent at first, later an ancestor of that), so whichever of them the 32-bit
// load returns -- the one from before this launch or one another lane has just stored -- root[i] moves to an
// ancestor of i that is at least as far as the synchronous round would take it, and a 32-bit aligned access
// cannot tear.  For the same reason the accesses are relaxed atomics of workgroup scope, which compile to plain
// cached loads and stores: freshness is not needed, and a wider scope would send the many lanes of a basin that all
// read the same few near-root entries past the caches, one memory access each.  After k rounds root[i] skips min(2^k, its distance to the root) links, so ceil(log2(h w)) rounds
// finish the longest chain there can be.  A round that stores nothing leaves its flag clear and every later
// round returns at once: in a launch that stored nothing all loads saw values from earlier launches, so nothing
// is left to do.
__global__ __launch_bounds__(NT) void ws_jump_kernel(int32_t* root_all, long long hw, const int* prev_flag,
                                                     int* flag) {
  if (prev_flag && __hip_atomic_load(prev_flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0) return;
  int32_t* root = root_all + (long long)blockIdx.y * hw;
  bool changed = false;
  for (long long i = (long long)blockIdx.x * NT + threadIdx.x; i < hw; i += (long long)gridDim.x * NT) {
    const int a = __hip_atomic_load(root + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    if (a < 0 || a == (int)i) continue;
    EUNET_DASSERT((long long)a < hw);
    const int b = __hip_atomic_load(root + a, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    EUNET_DASSERT(b >= 0 && (long long)b < hw);
    if (b != a) {
      __hip_atomic_store(root + i, b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
      changed = true;
    }
  }
  // the flag only ever goes from 0 to 1: a wave that already sees it set has nothing to add (thousands of waves
  // adding to one word are served one after the other)
  if (__any(changed) && (threadIdx.x & 63) == 0 && __hip_atomic_load(flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0)
    atomicOr(flag, 1);
}

// grid (gx, p), whole waves.  first[r] = the smallest pixel index of the basin of root r.  The lanes of a wave hold
// consecutive pixels, so within a run of one root the first lane has the smallest index and adds alone.
__global__ __launch_bounds__(NT) void ws_first_kernel(const int32_t* root_all, long long hw, int32_t* first_all) {
  const int32_t* root = root_all + (long long)blockIdx.y * hw;
  int32_t* first = first_all + (long long)blockIdx.y * hw;
  const long long blocks = (hw + NT - 1) / NT;
  for (long long blk = blockIdx.x; blk < blocks; blk += gridDim.x) {
    const long long i = blk * NT + threadIdx.x;
    const int r = i < hw ? root[i] : -1;
    const int prev = __shfl_up(r, 1, 64);
    if (r >= 0 && ((threadIdx.x & 63) == 0 || prev != r)) {
      EUNET_DASSERT((long long)r < hw && root[r] == r);
      atomicMin(first + r, (int)i);
    }
  }
}

// prefix sum over the first-pixel flags, as instances.hip numbers components: per-block counts of NT consecutive
// pixels, one block per plane scanning its counts, per-block ranks (labelmap.h).
__device__ __forceinline__ bool is_first(const int32_t* root, const int32_t* first, long long hw, long long i) {
  if (i >= hw) return false;
  const int r = root[i];
  if (r < 0) return false;
  EUNET_DASSERT((long long)r < hw);
  return first[r] == (int)i;
}

// grid (nbp, p), nbp = ceil(hw / NT)
__global__ __launch_bounds__(NT) void ws_count_kernel(const int32_t* root_all, const int32_t* first_all, long long hw,
                                                      int* block_count) {
  const long long base = (long long)blockIdx.y * hw;
  int tot;
  block_exclusive_scan_flag(is_first(root_all + base, first_all + base, hw, (long long)blockIdx.x * NT + threadIdx.x),
                            &tot);
  if (threadIdx.x == 0) block_count[(long long)blockIdx.y * gridDim.x + blockIdx.x] = tot;
}

// grid (nbp, p): basin[first pixel] = 1 + the number of first pixels before it in its plane
__global__ __launch_bounds__(NT) void ws_rank_kernel(const int32_t* root_all, const int32_t* first_all, long long hw,
                                                     const int* block_off, int32_t* basin_all) {
  const long long base = (long long)blockIdx.y * hw;
  const long long i = (long long)blockIdx.x * NT + threadIdx.x;
  const bool f = is_first(root_all + base, first_all + base, hw, i);
  int tot;
  const int before = block_exclusive_scan_flag(f, &tot);
  if (f) basin_all[base + i] = block_off[(long long)blockIdx.y * gridDim.x + blockIdx.x] + before + 1;
}

// grid (gx, p): every other pixel takes the number its basin's first pixel holds (first pixels are read here and
// written by no lane of this launch); background is 0
__global__ __launch_bounds__(NT) void ws_fill_kernel(const int32_t* root_all, const int32_t* first_all, long long hw,
                                                     int32_t* basin_all) {
  const long long base = (long long)blockIdx.y * hw;
  const int32_t* root = root_all + base;
  const int32_t* first = first_all + base;
  int32_t* basin = basin_all + base;
  for (long long i = (long long)blockIdx.x * NT + threadIdx.x; i < hw; i += (long long)gridDim.x * NT) {
    const int r = root[i];
    if (r < 0) {
      basin[i] = 0;
      continue;
    }
    EUNET_DASSERT((long long)r < hw);
    const int f = first[r];
    EUNET_DASSERT(f >= 0 && (long long)f <= i);
    if (f != (int)i) basin[i] = basin[f];
  }
}

// grid (gx, p): the root pixel of basin b of plane q writes slot offs[q] + b - 1
__global__ __launch_bounds__(NT) void ws_peaks_kernel(const int32_t* dist_all, const int32_t* root_all,
                                                      const int32_t* basin_all, long long hw, const int32_t* offs,
                                                      int nb_total, int32_t* broot, int32_t* bpeak) {
  const long long base = (long long)blockIdx.y * hw;
  const int off = offs[blockIdx.y];
  for (long long i = (long long)blockIdx.x * NT + threadIdx.x; i < hw; i += (long long)gridDim.x * NT) {
    if (root_all[base + i] != (int)i) continue;
    const int g = off + basin_all[base + i] - 1;
    EUNET_DASSERT(g >= off && g < nb_total);
    if (g < 0 || g >= nb_total) continue;
    broot[g] = (int)i;
    bpeak[g] = dist_all[base + i];
  }
}

// Every lane brings at most one (pair, value).  A run of a basin border puts the same pair on many lanes of a wave:
// the lanes that share the first pending lane's pair are reduced with a wave maximum and inserted once, at most
// twice in a row; what is left inserts for itself.  A maximum: exact either way.  Whole waves only.
__device__ __forceinline__ void wave_put(const Table& t, bool has, unsigned long long key, int val) {
  const int lane = threadIdx.x & 63;
  unsigned long long todo = __ballot(has);
#pragma unroll 1
  for (int round = 0; round < 2 && todo; ++round) {
    const int lead = __ffsll((long long)todo) - 1;
    const unsigned long long lk = __shfl(key, lead, 64);
    const bool mate = has && key == lk;
    const unsigned long long mates = __ballot(mate);
    if (__popcll(mates) < MIN_MATES) break;
    const int m = wave_max(mate ? val : 0);
    if (lane == lead) table_update<TableMax>(t, lk, m);
    has = has && !mate;
    todo &= ~mates;
  }
  if (has) table_update<TableMax>(t, key, val);
}

// grid (gx, p), whole waves.  Each foreground pixel looks at its E, SW, S and SE neighbours: every unordered pair of
// 8-adjacent pixels is seen exactly once.
__global__ __launch_bounds__(NT) void ws_saddles_kernel(const int32_t* dist_all, const int32_t* basin_all, int h, int w,
                                                        const int32_t* offs, Table t) {
  const long long hw = (long long)h * w;
  const int32_t* d = dist_all + (long long)blockIdx.y * hw;
  const int32_t* basin = basin_all + (long long)blockIdx.y * hw;
  const unsigned off = (unsigned)offs[blockIdx.y];
  const long long blocks = (hw + NT - 1) / NT;
  for (long long blk = blockIdx.x; blk < blocks; blk += gridDim.x) {
    const long long i = blk * NT + threadIdx.x;
    const bool in = i < hw;
    const int y = in ? (int)(i / w) : 0, x = in ? (int)(i - (long long)y * w) : 0;
    const int bp = in ? basin[i] : 0;
    const int dp = bp > 0 ? d[i] : 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int dx = k == 0 ? 1 : k - 2, dy = k == 0 ? 0 : 1;  // E, SW, S, SE
      const int xx = x + dx, yy = y + dy;
      bool has = false;
      unsigned long long key = 0ull;
      int val = 0;
      if (bp > 0 && xx >= 0 && xx < w && yy < h) {
        const long long q = (long long)yy * w + xx;
        EUNET_DASSERT(q >= 0 && q < hw);
        const int bq = basin[q];
        if (bq > 0 && bq != bp) {
          const int dq = d[q];
          const unsigned a = off + (unsigned)(bp < bq ? bp : bq) - 1u, b = off + (unsigned)(bp < bq ? bq : bp) - 1u;
          key = ((unsigned long long)a << 32) | b;
          val = dp < dq ? dp : dq;
          has = true;
        }
      }
      wave_put(t, has, key, val);
    }
  }
}

// grid (gx, p), whole waves.  ids[i] = table[offs[plane] + basin[i] - 1] (in place when ids == basin: a lane reads and
// writes its own pixel only); areas[plane][id - 1] += the length of every run of the id within a wave: one atomic by
// the run's first lane (the lanes of a wave hold consecutive pixels, so a cell's row is one run).
__global__ __launch_bounds__(NT) void ws_relabel_kernel(const int32_t* basin_all, long long hw, const int32_t* offs,
                                                        const int32_t* table, int nb_total, int32_t* ids_all,
                                                        int32_t* areas_all, int amax) {
  const long long base = (long long)blockIdx.y * hw;
  const int off = offs[blockIdx.y];
  int32_t* areas = areas_all + (long long)blockIdx.y * amax;
  const long long blocks = (hw + NT - 1) / NT;
  for (long long blk = blockIdx.x; blk < blocks; blk += gridDim.x) {
    const long long i = blk * NT + threadIdx.x;
    int id = 0;
    if (i < hw) {
      const int b = basin_all[base + i];
      if (b > 0) {
        const int g = off + b - 1;
        EUNET_DASSERT(g >= 0 && g < nb_total);
        if (g >= 0 && g < nb_total) id = table[g];
      }
      ids_all[base + i] = id;
    }
    EUNET_DASSERT(id >= 0 && id <= amax);
    const int lane = threadIdx.x & 63;
    const int prev = __shfl_up(id, 1, 64);
    const bool head = lane == 0 || prev != id;
    const unsigned long long heads = __ballot(head);
    if (head && id > 0 && id <= amax) {
      const unsigned long long above = lane == 63 ? 0ull : heads >> (lane + 1);
      atomicAdd(areas + id - 1, above ? __ffsll((long long)above) : 64 - lane);  // to the next head, or the wave's end
    }
  }
}

int jump_rounds(long long hw) {
  int r = 0;
  while ((1ll << r) < hw) ++r;
  return r + 1;  // ceil(log2(hw)) rounds finish every chain; one more so that a 1-pixel plane has a round too
}

}  // namespace

extern "C" {

int eunet_watershed_workspace_bytes(int p, int h, int w, size_t* bytes) {
  EUNET_REQUIRE(bytes, "watershed_workspace_bytes: null pointer");
  EUNET_REQUIRE(plane_stack_ok(p, h, w, true),
                "watershed_workspace_bytes: bad shape (p 1..65535, h and w 1..%d, p h w < 2^31)", EUNET_EDT_MAX_SIDE);
  const long long hw = (long long)h * w;
  const long long nbp = (hw + NT - 1) / NT;
  *bytes = sizeof(int32_t) * (size_t)(2 * (long long)p * hw + (long long)p * nbp + EUNET_WATERSHED_FLAG_WORDS);
  return EUNET_OK;
}

int eunet_watershed_basins(const int32_t* dist, int p, int h, int w, int32_t* basin, int32_t* counts, int32_t* ws,
                           void* stream) {
  EUNET_REQUIRE(dist && basin && counts && ws, "watershed_basins: null pointer");
  EUNET_REQUIRE(plane_stack_ok(p, h, w, true), "watershed_basins: bad shape (p 1..65535, h and w 1..%d, p h w < 2^31)",
                EUNET_EDT_MAX_SIDE);
  EUNET_REQUIRE(dist != basin, "watershed_basins: not in place");
  const hipStream_t s = (hipStream_t)stream;
  const long long hw = (long long)h * w, total = (long long)p * hw;
  const long long nbp = (hw + NT - 1) / NT;
  int32_t* root = ws;
  int32_t* first = ws + total;
  int* block_count = ws + 2 * total;
  int* flags = ws + 2 * total + (long long)p * nbp;
  const int rounds = jump_rounds(hw);
  static_assert(EUNET_WATERSHED_FLAG_WORDS >= 28, "a flag per round of a 8192 x 8192 plane");
  if (!fill_async(flags, 0, sizeof(int) * EUNET_WATERSHED_FLAG_WORDS, s, "watershed_basins") ||
      !fill_async(first, 0x7f, sizeof(int32_t) * (size_t)total, s, "watershed_basins"))
    return EUNET_ERR_HIP;
  ws_up_kernel<<<dim3((unsigned)cdiv(w, UP_W), (unsigned)cdiv(h, UP_ROWS), (unsigned)p), UP_NT, 0, s>>>(dist, h, w,
                                                                                                       root);
  const dim3 gp(grid_for(hw, GRID_CAP), (unsigned)p);
  for (int r = 0; r < rounds; ++r)
    ws_jump_kernel<<<gp, NT, 0, s>>>(root, hw, r ? flags + r - 1 : nullptr, flags + r);
  ws_first_kernel<<<gp, NT, 0, s>>>(root, hw, first);
  const dim3 gb((unsigned)nbp, (unsigned)p);
  ws_count_kernel<<<gb, NT, 0, s>>>(root, first, hw, block_count);
  scan_block_counts_kernel<NT><<<(unsigned)p, NT, 0, s>>>(block_count, (int)nbp, counts);
  ws_rank_kernel<<<gb, NT, 0, s>>>(root, first, hw, block_count, basin);
  ws_fill_kernel<<<gp, NT, 0, s>>>(root, first, hw, basin);
  EUNET_LAUNCH_CHECK("watershed_basins");
  return EUNET_OK;
}

int eunet_watershed_peaks(const int32_t* dist, const int32_t* basin, const int32_t* ws, int p, int h, int w,
                          const int32_t* offs, int nb_total, int32_t* root, int32_t* peak, void* stream) {
  EUNET_REQUIRE(dist && basin && ws && offs && root && peak, "watershed_peaks: null pointer");
  EUNET_REQUIRE(plane_stack_ok(p, h, w, true) && nb_total >= 1, "watershed_peaks: bad shape");
  const long long hw = (long long)h * w;
  ws_peaks_kernel<<<dim3(grid_for(hw, GRID_CAP), (unsigned)p), NT, 0, (hipStream_t)stream>>>(
      dist, ws, basin, hw, offs, nb_total, root, peak);
  EUNET_LAUNCH_CHECK("watershed_peaks");
  return EUNET_OK;
}

int eunet_watershed_saddles(const int32_t* dist, const int32_t* basin, int p, int h, int w, const int32_t* offs,
                            int64_t* keys, int32_t* vals, long long capacity, int32_t* overflow, void* stream) {
  EUNET_REQUIRE(dist && basin && offs && keys && vals && overflow, "watershed_saddles: null pointer");
  EUNET_REQUIRE(plane_stack_ok(p, h, w, true), "watershed_saddles: bad shape");
  EUNET_REQUIRE(((uintptr_t)keys & 7u) == 0, "watershed_saddles: misaligned keys");
  const hipStream_t s = (hipStream_t)stream;
  Table t;
  const int rc = table_init("watershed_saddles", keys, vals, capacity, overflow, s, &t);
  if (rc != EUNET_OK) return rc;
  ws_saddles_kernel<<<dim3(grid_for((long long)h * w, GRID_CAP), (unsigned)p), NT, 0, s>>>(dist, basin, h, w, offs, t);
  EUNET_LAUNCH_CHECK("watershed_saddles");
  return EUNET_OK;
}

int eunet_watershed_relabel(const int32_t* basin, int p, int h, int w, const int32_t* offs, const int32_t* table,
                            int nb_total, int32_t* ids, int32_t* areas, int amax, void* stream) {
  EUNET_REQUIRE(basin && offs && table && ids && areas, "watershed_relabel: null pointer");
  EUNET_REQUIRE(plane_stack_ok(p, h, w, true) && nb_total >= 1 && amax >= 1, "watershed_relabel: bad shape");
  const hipStream_t s = (hipStream_t)stream;
  if (!fill_async(areas, 0, sizeof(int32_t) * (size_t)p * (size_t)amax, s, "watershed_relabel")) return EUNET_ERR_HIP;
  const long long hw = (long long)h * w;
  ws_relabel_kernel<<<dim3(grid_for(hw, GRID_CAP), (unsigned)p), NT, 0, s>>>(basin, hw, offs, table, nb_total, ids, areas,
                                                                             amax);
  EUNET_LAUNCH_CHECK("watershed_relabel");
  return EUNET_OK;
}

}  // extern "C"
