// Label-map instance metrics: the sparse contingency table of two label maps, and the label map of a mask stack.
//
// Every instance-level score of two segmentations given as integer id maps (Panoptic Quality, the Aggregated Jaccard
// Index, object Dice, SEG, the F1 sweep; eunet/metrics.py) is a function of one table: for each pair (id in a, id in
// b) the number of pixels that carry both.  The definitions are in include/eunet.h ("label-map instance metrics").
//   pairs_kernel        one pass over both maps, 16 bytes per lane and load; a wave holds 256 consecutive pixels, four
//                       per lane; the first pixel of every run of one key inserts (key, run length) into an
//                       open-addressing hash table (atomicCAS claims the slot, an integer atomicAdd counts)
//   labels_from_stack_kernel   uint8 planes + an id per plane -> one int32 id map, the last selected plane wins
// Every loop is bounded by the shapes or by a constant, every result is an integer and independent of the order in
// which the atomics land.
#include "common.h"
#include "labelmap.h"

EUNET_DEBUG_UNIT(pairs)

namespace {

constexpr int NT = 256;
static_assert(NT == LM_NT, "labelmap.h sizes blocks of NT");
constexpr int GRID_CAP = 2048;           // blocks of a grid-stride launch
constexpr int PV = 4;                    // pixels a lane holds
constexpr int WAVE_PX = 64 * PV;         // pixels a wave holds
constexpr long long ID_MAX = EUNET_PAIRS_MAX_ID;

// PV consecutive ids starting at element i (i a multiple of PV).  VEC: the base pointer is 16-byte aligned, so a
// lane whose PV pixels all lie inside reads them 16 bytes at a time; the last lane of the map reads what is there.
template <typename T, bool VEC>
__device__ __forceinline__ void load_ids(const T* __restrict__ src, long long i, long long total, long long (&v)[PV]) {
  if (VEC && i + PV <= total) {
    if constexpr (sizeof(T) == 4) {
      const int4 q = *reinterpret_cast<const int4*>(src + i);
      v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
    } else {
      const longlong2 q0 = *reinterpret_cast<const longlong2*>(src + i);
      const longlong2 q1 = *reinterpret_cast<const longlong2*>(src + i + 2);
      v[0] = q0.x; v[1] = q0.y; v[2] = q1.x; v[3] = q1.y;
    }
  } else {
#pragma unroll
    for (int j = 0; j < PV; ++j) v[j] = i + j < total ? (long long)src[i + j] : -1ll;  // past the end: not counted
  }
}

// grid-stride over chunks of WAVE_PX pixels of the p planes laid end to end, one chunk per wave and round.  Whole
// waves only: the shuffles and ballots need every lane, lanes past the end hold uncounted pixels and never insert.
// A boundary is a pixel whose key differs from the one before it in the chunk (the chunk's first pixel is one); a
// boundary with a counted key is a run head, its run ends at the next boundary or at the chunk's end.  Every counted
// pixel lies in exactly one run, so the table is exact whatever the pattern: noise degrades to one insert per pixel.
template <typename TA, typename TB, bool VEC>
__global__ __launch_bounds__(NT) void pairs_kernel(const TA* __restrict__ a, const TB* __restrict__ b, int p,
                                                   long long hw, Table t, unsigned long long* invalid) {
  const long long total = (long long)p * hw;
  const long long chunks = (total + WAVE_PX - 1) / WAVE_PX;
  const int lane = threadIdx.x & 63;
  const long long wave = (long long)blockIdx.x * (NT / 64) + (threadIdx.x >> 6);
  const long long waves = (long long)gridDim.x * (NT / 64);
  unsigned bad = 0;
  for (long long c = wave; c < chunks; c += waves) {
    const long long i0 = c * WAVE_PX + (long long)lane * PV;
    long long va[PV], vb[PV];
    load_ids<TA, VEC>(a, i0, total, va);
    load_ids<TB, VEC>(b, i0, total, vb);
    long long plane = i0 < total ? i0 / hw : 0;
    long long rem = i0 < total ? i0 - plane * hw : 0;
    unsigned long long key[PV];
#pragma unroll
    for (int j = 0; j < PV; ++j) {
      if (rem >= hw) {  // rem <= hw here, as it grows by one per pixel: the next plane starts at this pixel
        rem = 0;
        ++plane;
      }
      ++rem;
      key[j] = EMPTY;
      if (va[j] < 0 || vb[j] < 0) continue;  // ignored (and everything past the end)
      if (va[j] > ID_MAX || vb[j] > ID_MAX) {
        ++bad;
        continue;
      }
      if (va[j] == 0 && vb[j] == 0) continue;
      EUNET_DASSERT(i0 + j < total && plane >= 0 && plane < p);
      key[j] = ((unsigned long long)plane << 48) | ((unsigned long long)va[j] << 24) | (unsigned long long)vb[j];
    }
    unsigned long long prev = __shfl_up(key[PV - 1], 1, 64);
    unsigned bm = 0;  // bit j: pixel j of this lane is a boundary
#pragma unroll
    for (int j = 0; j < PV; ++j) {
      if ((j == 0 && lane == 0) || key[j] != prev) bm |= 1u << j;
      prev = key[j];
    }
    // the first boundary after this lane's pixels: in lane nl, at its pixel ctz(nbm)
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
      EUNET_DASSERT(len >= 1 && lane * PV + j + len <= WAVE_PX && i0 + j + len <= total);
      table_update<TableAdd>(t, key[j], len);
    }
  }
  bad = wave_sum(bad);
  if (lane == 0 && bad) atomicAdd(invalid, (unsigned long long)bad);
}

// ---- mask stack -> id map.  LV pixels per lane: 16 with one 16-byte load per plane, or 1.
template <int LV>
__global__ __launch_bounds__(NT) void labels_from_stack_kernel(const uint8_t* __restrict__ masks, int n, long long hw,
                                                               const int32_t* __restrict__ ids,
                                                               const uint8_t* __restrict__ ignore,
                                                               int32_t* __restrict__ out,
                                                               unsigned long long* overlap) {
  const long long units = (hw + LV - 1) / LV;
  unsigned over = 0;
  for (long long u = (long long)blockIdx.x * NT + threadIdx.x; u < units; u += (long long)gridDim.x * NT) {
    const long long i = u * LV;  // LV > 1 only when LV divides hw: a unit never crosses the end
    EUNET_DASSERT(i + LV <= hw);
    int32_t v[LV];
#pragma unroll
    for (int k = 0; k < LV; ++k) v[k] = 0;
    unsigned seen = 0, multi = 0;  // bit k: pixel k is claimed by a selected plane / by more than one
    for (int j = 0; j < n; ++j) {
      const int32_t id = ids[j];  // uniform over the launch
      if (id <= 0) continue;
      const uint8_t* m = masks + (long long)j * hw + i;
      unsigned set = 0;
      if constexpr (LV == 16) {
        const uint4 q = *reinterpret_cast<const uint4*>(m);
        const unsigned wds[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
        for (int k = 0; k < 16; ++k)
          if ((wds[k >> 2] >> (8 * (k & 3))) & 0xffu) set |= 1u << k;
      } else {
        set = m[0] != 0 ? 1u : 0u;
      }
      multi |= seen & set;
      seen |= set;
#pragma unroll
      for (int k = 0; k < LV; ++k)
        if ((set >> k) & 1u) v[k] = id;  // a later plane overwrites an earlier one
    }
    over += (unsigned)__popc(multi);
    if (ignore) {
      if constexpr (LV == 16) {
        const uint4 q = *reinterpret_cast<const uint4*>(ignore + i);
        const unsigned wds[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
        for (int k = 0; k < 16; ++k)
          if ((wds[k >> 2] >> (8 * (k & 3))) & 0xffu) v[k] = -1;
      } else {
        if (ignore[i] != 0) v[0] = -1;
      }
    }
    if constexpr (LV == 16) {
#pragma unroll
      for (int k = 0; k < 16; k += 4)
        *reinterpret_cast<int4*>(out + i + k) = make_int4(v[k], v[k + 1], v[k + 2], v[k + 3]);
    } else {
      out[i] = v[0];
    }
  }
  over = wave_sum(over);
  if ((threadIdx.x & 63) == 0 && over) atomicAdd(overlap, (unsigned long long)over);
}

template <typename TA, typename TB>
void launch_pairs(const void* a, const void* b, int p, long long hw, const Table& t, int64_t* invalid, hipStream_t s) {
  const long long chunks = ((long long)p * hw + WAVE_PX - 1) / WAVE_PX;
  const unsigned g = grid_for(chunks * 64, GRID_CAP);
  const bool vec = (((uintptr_t)a | (uintptr_t)b) & 15u) == 0;
  if (vec)
    pairs_kernel<TA, TB, true><<<g, NT, 0, s>>>((const TA*)a, (const TB*)b, p, hw, t, (unsigned long long*)invalid);
  else
    pairs_kernel<TA, TB, false><<<g, NT, 0, s>>>((const TA*)a, (const TB*)b, p, hw, t, (unsigned long long*)invalid);
}

}  // namespace

extern "C" {

int eunet_label_pairs(const void* a, int a_bytes, const void* b, int b_bytes, int p, int h, int w, int64_t* keys,
                      int32_t* counts, long long capacity, int32_t* overflow, int64_t* invalid, void* stream) {
  EUNET_REQUIRE(a && b && keys && counts && overflow && invalid, "label_pairs: null pointer");
  EUNET_REQUIRE((a_bytes == 4 || a_bytes == 8) && (b_bytes == 4 || b_bytes == 8),
                "label_pairs: int32 or int64 maps (a_bytes, b_bytes 4 or 8)");
  EUNET_REQUIRE(plane_stack_ok(p, h, w, true), "label_pairs: bad shape (p 1..65535, h and w 1..%d, p h w < 2^31)",
                EUNET_EDT_MAX_SIDE);
  EUNET_REQUIRE(((uintptr_t)keys & 7u) == 0 && ((uintptr_t)invalid & 7u) == 0 &&
                    ((uintptr_t)a & (uintptr_t)(a_bytes - 1)) == 0 && ((uintptr_t)b & (uintptr_t)(b_bytes - 1)) == 0,
                "label_pairs: misaligned pointer");
  const hipStream_t s = (hipStream_t)stream;
  Table t;
  const int rc = table_init("label_pairs", keys, counts, capacity, overflow, s, &t);
  if (rc != EUNET_OK) return rc;
  if (!fill_async(invalid, 0, sizeof(int64_t), s, "label_pairs")) return EUNET_ERR_HIP;
  const long long hw = (long long)h * w;
  if (a_bytes == 4 && b_bytes == 4) launch_pairs<int32_t, int32_t>(a, b, p, hw, t, invalid, s);
  else if (a_bytes == 4) launch_pairs<int32_t, int64_t>(a, b, p, hw, t, invalid, s);
  else if (b_bytes == 4) launch_pairs<int64_t, int32_t>(a, b, p, hw, t, invalid, s);
  else launch_pairs<int64_t, int64_t>(a, b, p, hw, t, invalid, s);
  EUNET_LAUNCH_CHECK("label_pairs");
  return EUNET_OK;
}

int eunet_labels_from_stack(const uint8_t* masks, int n, int h, int w, const int32_t* ids, const uint8_t* ignore,
                            int32_t* out, int64_t* overlap, void* stream) {
  EUNET_REQUIRE(out && overlap && n >= 0 && n <= 65535 && (n == 0 || (masks && ids)),
                "labels_from_stack: bad args (0 <= n <= 65535 planes)");
  EUNET_REQUIRE(h >= 1 && w >= 1 && (long long)h * w < (1ll << 31),
                "labels_from_stack: bad shape (h w < 2^31)");
  EUNET_REQUIRE(((uintptr_t)out & 3u) == 0 && ((uintptr_t)overlap & 7u) == 0, "labels_from_stack: misaligned pointer");
  const hipStream_t s = (hipStream_t)stream;
  if (!fill_async(overlap, 0, sizeof(int64_t), s, "labels_from_stack")) return EUNET_ERR_HIP;
  const long long hw = (long long)h * w;
  // 16 pixels per lane when every plane starts on a 16-byte boundary and no unit crosses the end
  const bool wide = hw % 16 == 0 && (((uintptr_t)masks | (uintptr_t)ignore | (uintptr_t)out) & 15u) == 0;
  if (wide)
    labels_from_stack_kernel<16><<<grid_for(hw / 16, GRID_CAP), NT, 0, s>>>(masks, n, hw, ids, ignore, out,
                                                                             (unsigned long long*)overlap);
  else
    labels_from_stack_kernel<1><<<grid_for(hw, GRID_CAP), NT, 0, s>>>(masks, n, hw, ids, ignore, out,
                                                                       (unsigned long long*)overlap);
  EUNET_LAUNCH_CHECK("labels_from_stack");
  return EUNET_OK;
}

}  // extern "C"
