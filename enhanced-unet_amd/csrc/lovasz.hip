// Lovasz-Softmax and Lovasz hinge losses (Berman, Triki, Blaschko, CVPR 2018) on a stable segmented radix sort.
//
// No reference line to cite: every loss of the reference is a sum over pixels.  The definition is the one in
// include/eunet.h ("Lovasz losses"): per segment (a class, or a class of one sample) the errors are ordered
// descending, the gradient of the Jaccard extension g_r is a closed form of the integer foreground count among the
// first r elements, and the segment loss is sum_r e_(r) g_r.
//
// Launches of a forward call, all on the caller's stream and all sized by the shape alone:
//   errors    one thread per pixel: the K errors and flags -> sort keys and payloads in segment-contiguous layout,
//             and one row of counts per block; a second launch sums the rows into the per-segment G (foreground),
//             V (valid) and the out-of-range targets
//   sort      lovasz_sort_pairs: four passes of 8 bits, least significant digit first, each pass three launches
//             (per-block digit histograms, a scan of every digit's row of block counts, a scatter).  A block owns
//             LZ_T consecutive pairs, a wave LZ_T / 4 consecutive ones of them, 64 at a time.  Equal digits of such a
//             round find each other with eight ballots (match), and their rank is the wave's running count of the
//             digit plus the number of peers on lower lanes: a position is a function of the input alone, no atomic
//             decides one, and equal keys keep their input order.
//   scan      the inclusive scan of the foreground bit over the sorted segment: per-block counts, labelmap.h's
//             scan_block_counts_kernel over them, then block_exclusive_scan_flag inside the block
//   gradient  (same launch as the last scan step) g_r from G, r and F_r in fp64, rounded once; g is scattered to the
//             element's own position in `weights`, and the block's fp64 sum of e g is one partial
//   finalize  one block: every segment's fp64 sum of its partials in a fixed order, the selection from G and V, the
//             means, and the per-segment factor table that the backward multiplies `weights` with
// The backward is one streaming pass on the skeleton of pixelloss.h.
#include "common.h"
#include "pixelloss.h"
#include "labelmap.h"

EUNET_DEBUG_UNIT(lovasz)

namespace {

constexpr int LZ_ITEMS = 8;              // pairs per thread of a sort or scan block
constexpr int LZ_T = LM_NT * LZ_ITEMS;   // pairs per block: 2048
constexpr int LZ_WAVE = LZ_ITEMS * 64;   // consecutive pairs per wave of a sort block
constexpr int LZ_BITS = 8, LZ_RADIX = 1 << LZ_BITS, LZ_PASSES = 32 / LZ_BITS;
constexpr int LZ_MAX_SEG = 64 * 3;       // N <= 64, K <= 3
constexpr uint32_t LZ_KEY_IGNORED = 0xFFFFFFFFu;
static_assert(LZ_RADIX == LM_NT, "one thread per digit");

// ---------------------------------------------------------------------------
// keys: ascending key = descending error; NaN first (key 0, as torch.sort(descending=True) places it), -0 as +0,
// an ignored element last (no error has the key 0xFFFFFFFF: its preimage is a NaN)
// ---------------------------------------------------------------------------
__device__ __forceinline__ uint32_t key_of(float e) {
  if (e != e) return 0u;
  uint32_t u = __float_as_uint(e);
  if (u == 0x80000000u) u = 0u;
  const uint32_t m = (u & 0x80000000u) ? ~u : (u | 0x80000000u);  // ascending with e
  return ~m;
}
__device__ __forceinline__ float error_of(uint32_t key) {
  if (key == 0u) return __uint_as_float(0x7FC00000u);
  const uint32_t m = ~key;
  return __uint_as_float((m & 0x80000000u) ? (m & 0x7FFFFFFFu) : ~m);
}

// the lanes of the wave whose digit equals this lane's, among the valid ones
__device__ __forceinline__ unsigned long long match_digit(unsigned d, bool valid) {
  unsigned long long m = __ballot(valid);
#pragma unroll
  for (int bit = 0; bit < LZ_BITS; ++bit) {
    const bool on = (d >> bit) & 1u;
    const unsigned long long b = __ballot(on);
    m &= on ? b : ~b;
  }
  return m;
}

// ---------------------------------------------------------------------------
// the sort: S segments of L pairs, segment on grid.y, LZ_T pairs per block
// ---------------------------------------------------------------------------
// first pair of this lane in its wave's run of LZ_WAVE pairs; round r adds 64 r
__device__ __forceinline__ long long sort_lane_base() {
  return (long long)blockIdx.x * LZ_T + (threadIdx.x >> 6) * LZ_WAVE + (threadIdx.x & 63);
}

// table [S][256][nb]: the number of keys of block b with the digit d
__global__ __launch_bounds__(LM_NT) void lz_hist_kernel(const uint32_t* keys, int L, int nb, int shift, int* table) {
  __shared__ int hist[LZ_RADIX];
  const int tid = threadIdx.x, lane = tid & 63, seg = blockIdx.y;
  hist[tid] = 0;
  __syncthreads();
  const uint32_t* k = keys + (long long)seg * L;
  const long long base = sort_lane_base();
#pragma unroll
  for (int r = 0; r < LZ_ITEMS; ++r) {
    const long long i = base + r * 64;
    const bool valid = i < L;
    const unsigned d = valid ? (k[i] >> shift) & (LZ_RADIX - 1) : 0u;
    const unsigned long long peers = match_digit(d, valid);
    // one add per digit and round, by its lowest lane: a count, whatever the order of the adds
    if (valid && (peers & ((1ull << lane) - 1ull)) == 0ull) atomicAdd(&hist[d], __popcll(peers));
  }
  __syncthreads();
  table[((long long)seg * LZ_RADIX + tid) * nb + blockIdx.x] = hist[tid];
}

// table: per (segment, digit) row the exclusive offsets over the blocks (scan_block_counts_kernel), dtot [S][256] the
// rows' totals.  dst = (keys of lower digits) + (keys of this digit in earlier blocks) + (in earlier waves of the
// block) + (earlier in the wave).
__global__ __launch_bounds__(LM_NT) void lz_scatter_kernel(const uint32_t* kin, const uint32_t* pin, uint32_t* kout,
                                                           uint32_t* pout, int L, int nb, int shift,
                                                           const int* table, const int32_t* dtot) {
  __shared__ int whist_s[LM_NT / 64][LZ_RADIX];
  __shared__ int wtot[LM_NT / 64];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, seg = blockIdx.y;
#pragma unroll
  for (int w = 0; w < LM_NT / 64; ++w) whist_s[w][tid] = 0;
  __syncthreads();
  volatile int* whist = whist_s[wv];  // this wave's running digit counts: read by all lanes, then written by the leaders
  const long long so = (long long)seg * L;
  const long long base = sort_lane_base();
  uint32_t key[LZ_ITEMS];
  int rank[LZ_ITEMS];
#pragma unroll
  for (int r = 0; r < LZ_ITEMS; ++r) {
    const long long i = base + r * 64;
    const bool valid = i < L;
    key[r] = valid ? kin[so + i] : 0u;
    const unsigned d = (key[r] >> shift) & (LZ_RADIX - 1);
    const unsigned long long peers = match_digit(d, valid);
    const int below = __popcll(peers & ((1ull << lane) - 1ull));
    const int prev = valid ? whist[d] : 0;
    __builtin_amdgcn_wave_barrier();
    rank[r] = prev + below;
    if (valid && below == 0) whist[d] = prev + __popcll(peers);
    __builtin_amdgcn_wave_barrier();
  }
  __syncthreads();
  // thread = digit: where the digit starts in the segment (exclusive scan of the 256 totals), then in this block,
  // then in each wave
  const int tot = dtot[seg * LZ_RADIX + tid];
  int inc = tot;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int t = __shfl_up(inc, o, 64);
    if (lane >= o) inc += t;
  }
  if (lane == 63) wtot[wv] = inc;
  __syncthreads();
  int start = inc - tot;
#pragma unroll
  for (int w = 0; w < LM_NT / 64; ++w)
    if (w < wv) start += wtot[w];
  start += table[((long long)seg * LZ_RADIX + tid) * nb + blockIdx.x];
#pragma unroll
  for (int w = 0; w < LM_NT / 64; ++w) {
    const int t = whist_s[w][tid];
    whist_s[w][tid] = start;
    start += t;
  }
  __syncthreads();
#pragma unroll
  for (int r = 0; r < LZ_ITEMS; ++r) {
    const long long i = base + r * 64;
    if (i < L) {
      const unsigned d = (key[r] >> shift) & (LZ_RADIX - 1);
      const int dst = whist_s[wv][d] + rank[r];
      EUNET_DASSERT(dst >= 0 && dst < L);
      if ((unsigned)dst < (unsigned)L) {  // a store is never issued outside the segment
        kout[so + dst] = key[r];
        pout[so + dst] = pin[so + i];
      }
    }
  }
}

inline int lz_blocks(int l) { return (int)(((long long)l + LZ_T - 1) / LZ_T); }
inline size_t lz_align(size_t b) { return (b + 255) & ~(size_t)255; }

// the sort's own workspace: the second pair of buffers, the block x digit table and the digit totals
struct SortWs {
  size_t keys, pay, table, dtot, total;
};
inline SortWs sort_ws(int s, int l) {
  SortWs w;
  const size_t pairs = lz_align((size_t)s * (size_t)l * 4);
  w.keys = 0;
  w.pay = pairs;
  w.table = 2 * pairs;
  w.dtot = w.table + lz_align((size_t)s * LZ_RADIX * lz_blocks(l) * 4);
  w.total = w.dtot + lz_align((size_t)s * LZ_RADIX * 4);
  return w;
}

// Sorts the S segments of L (key, payload) pairs each, in place, ascending by key, equal keys in input order.
// workspace: sort_ws(S, L).total bytes.  Twelve launches; no host synchronisation.
int lovasz_sort_pairs(uint32_t* keys, uint32_t* payload, int S, int L, void* workspace, hipStream_t stream) {
  const SortWs w = sort_ws(S, L);
  char* ws = (char*)workspace;
  uint32_t* k[2] = {keys, (uint32_t*)(ws + w.keys)};
  uint32_t* p[2] = {payload, (uint32_t*)(ws + w.pay)};
  int* table = (int*)(ws + w.table);
  int32_t* dtot = (int32_t*)(ws + w.dtot);
  const int nb = lz_blocks(L);
  const dim3 grid(nb, S);
  static_assert(LZ_PASSES % 2 == 0, "the result lands in the caller's buffers");
  for (int pass = 0; pass < LZ_PASSES; ++pass) {
    const int a = pass & 1, shift = pass * LZ_BITS;
    lz_hist_kernel<<<grid, LM_NT, 0, stream>>>(k[a], L, nb, shift, table);
    scan_block_counts_kernel<LM_NT><<<S * LZ_RADIX, LM_NT, 0, stream>>>(table, nb, dtot);
    lz_scatter_kernel<<<grid, LM_NT, 0, stream>>>(k[a], p[a], k[a ^ 1], p[a ^ 1], L, nb, shift, table, dtot);
  }
  return eunet::check_launch("lovasz_sort_pairs");
}

// ---------------------------------------------------------------------------
// counts: every block writes one row of integers, lz_count_kernel sums the rows of a segment.  (One atomic per wave
// and counter on a handful of addresses took longer than the sort.)
// ---------------------------------------------------------------------------
// the block's sums of acc[] -> row[0..NV): in the wave, then the four waves
template <int NV>
__device__ __forceinline__ void block_count_row(const int (&acc)[NV], int* row) {
  static_assert(LM_NT == 256 && PL_NT == 256, "four waves");
  __shared__ int red[4][NV];
  const int tid = threadIdx.x;
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const int v = wave_sum(acc[i]);
    if ((tid & 63) == 0) red[tid >> 6][i] = v;
  }
  __syncthreads();
  if (tid < NV) row[tid] = red[0][tid] + red[1][tid] + red[2][tid] + red[3][tid];
}

// grid (S + 1), rows [groups][per][width]: block s < S sums the `per` rows of its group (s / K, or the one group)
// in the columns s % K (-> G) and K (-> V) into cnt [S][2]; block S sums column K + 1 of every row into cnt[2 S]
// (cnt holds 2 S + 2 words)
__global__ __launch_bounds__(LM_NT) void lz_count_kernel(const int* cpart, int groups, int per, int width, int K,
                                                         int S, int* cnt) {
  const int s = blockIdx.x, tid = threadIdx.x;
  const bool last = s == S;
  const int grp = last || groups == 1 ? 0 : s / K;
  const long long rows = last ? (long long)groups * per : per;
  const int* base = cpart + (long long)grp * per * width;
  int acc[2] = {0, 0};
  for (long long r = tid; r < rows; r += LM_NT) {
    acc[0] += base[r * width + (last ? K + 1 : s % K)];
    acc[1] += last ? 0 : base[r * width + K];
  }
  block_count_row<2>(acc, cnt + 2 * s);  // block S: cnt[2 S] and a spare word after it
}

// ---------------------------------------------------------------------------
// errors and flags
// ---------------------------------------------------------------------------
// flag: 0 background, 1 foreground, 2 ignored (target == ignore_index) or out of range (*bad set); e = 0 where 2
template <int K, bool HINGE>
__device__ __forceinline__ void px_errors(const float (&x)[K], int64_t traw, int ignore_index, float (&e)[K],
                                          int (&flag)[K], bool* bad) {
  const bool ign = traw == (int64_t)ignore_index;
  // the rule of bce_dice's classify / target_of: K = 1 is "foreground" (any target >= 0, on where >= 1)
  const bool inrange = (HINGE && K == 1) ? traw >= 0 : (traw >= 0 && traw < K);
  *bad = !ign && !inrange;
  float p[K];
  if (!HINGE) softmax_px<K>(x, p);
#pragma unroll
  for (int c = 0; c < K; ++c) {
    const bool fg = (HINGE && K == 1) ? traw >= 1 : traw == (int64_t)c;
    const float f = fg ? 1.f : 0.f;
    const float v = HINGE ? 1.f - x[c] * (2.f * f - 1.f) : fabsf(f - p[c]);
    const bool skip = ign || !inrange;
    e[c] = skip ? 0.f : v;
    flag[c] = skip ? 2 : (fg ? 1 : 0);
  }
}

// grid (tiles, N).  errors / flags [N][K][HW] and keys / pay [S][L] are each optional (null: not written), and so is
// cpart [N][tiles][K + 2]: the block's foreground count per class, its valid pixels and its out-of-range targets.
template <int K, bool HINGE>
__global__ __launch_bounds__(PL_NT) void lz_errors_kernel(const float* logits, const int64_t* target, int N, int HW,
                                                          int per_image, int ignore_index, float* errors,
                                                          uint8_t* flags, uint32_t* keys, uint32_t* pay,
                                                          int* cpart) {
  const int n = blockIdx.y;
  const float* lg = logits + (long long)n * K * HW;
  const int64_t* tg = target + (long long)n * HW;
  const long long L = per_image ? HW : (long long)N * HW;
  int acc[K + 2];  // G per class, V, out-of-range targets
#pragma unroll
  for (int i = 0; i < K + 2; ++i) acc[i] = 0;
  pl_tile_visit<false>(HW, [&](int p) {
    float x[K], e[K];
    int flag[K];
    bool bad;
    pl_load<K>(lg, HW, x, p);
    px_errors<K, HINGE>(x, tg[p], ignore_index, e, flag, &bad);
    acc[K] += flag[0] != 2;
    acc[K + 1] += bad;
#pragma unroll
    for (int c = 0; c < K; ++c) {
      acc[c] += flag[c] == 1;
      const long long o = ((long long)n * K + c) * HW + p;
      if (errors) errors[o] = e[c];
      if (flags) flags[o] = (uint8_t)flag[c];
      if (keys) {
        const int seg = per_image ? n * K + c : c;
        const long long idx = per_image ? p : (long long)n * HW + p;
        EUNET_DASSERT(idx < L);
        keys[seg * L + idx] = flag[c] == 2 ? LZ_KEY_IGNORED : key_of(e[c]);
        pay[seg * L + idx] = ((uint32_t)idx << 1) | (uint32_t)(flag[c] == 1);
      }
    }
  });
  if (cpart) block_count_row<K + 2>(acc, cpart + ((long long)n * gridDim.x + blockIdx.x) * (K + 2));
}

// grid (nb, S): errors and flags already in segment layout [S][L] (eunet_lovasz_sort)
__global__ __launch_bounds__(LM_NT) void lz_keys_kernel(const float* errors, const uint8_t* flags, int L,
                                                        uint32_t* keys, uint32_t* pay, int* cpart) {
  const int seg = blockIdx.y;
  const long long so = (long long)seg * L;
  int acc[3] = {0, 0, 0};  // G, V, and the column of the out-of-range targets (none here)
#pragma unroll
  for (int r = 0; r < LZ_ITEMS; ++r) {
    const long long i = (long long)blockIdx.x * LZ_T + r * LM_NT + threadIdx.x;
    if (i < L) {
      const int f = flags[so + i];
      keys[so + i] = f >= 2 ? LZ_KEY_IGNORED : key_of(errors[so + i]);
      pay[so + i] = ((uint32_t)i << 1) | (uint32_t)(f == 1);
      acc[0] += f == 1;
      acc[1] += f < 2;
    }
  }
  block_count_row<3>(acc, cpart + ((long long)seg * gridDim.x + blockIdx.x) * 3);
}

// ---------------------------------------------------------------------------
// scan of the foreground bit and the Lovasz gradient; grid (nb, S), element r LM_NT + tid of the block in round r
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(LM_NT) void lz_fgcount_kernel(const uint32_t* pay, int L, int nb, const int* cnt,
                                                           int* block_count) {
  __shared__ int wave_tot[LM_NT / 64];
  const int seg = blockIdx.y, tid = threadIdx.x;
  const int V = cnt[seg * 2 + 1];
  const uint32_t* p = pay + (long long)seg * L;
  int c = 0;
#pragma unroll
  for (int r = 0; r < LZ_ITEMS; ++r) {
    const long long i = (long long)blockIdx.x * LZ_T + r * LM_NT + tid;
    if (i < V) c += (int)(p[i] & 1u);  // V <= L
  }
  c = wave_sum(c);
  if ((tid & 63) == 0) wave_tot[tid >> 6] = c;
  __syncthreads();
  if (tid == 0) block_count[(long long)seg * nb + blockIdx.x] = wave_tot[0] + wave_tot[1] + wave_tot[2] + wave_tot[3];
}

// block_count: exclusive over the segment's blocks.  g goes to weights at the element's own position: seg L + idx
// (by_class = 0: segments are [N][K] planes, or the caller's own [S][L]) or plane (n, seg) of [N][K][HW] with
// n = idx / HW (by_class = 1: segments are classes over the batch).  part [S][nb]: the block's fp64 sum of e g.
__global__ __launch_bounds__(LM_NT) void lz_grad_kernel(const uint32_t* keys, const uint32_t* pay, int L, int nb,
                                                        const int* cnt, const int* block_count, int hinge,
                                                        int by_class, int K, int HW, int32_t* order, float* weights,
                                                        double* part) {
  __shared__ double red[LM_NT / 64];
  const int seg = blockIdx.y, tid = threadIdx.x;
  const long long so = (long long)seg * L;
  const int G = cnt[seg * 2], V = cnt[seg * 2 + 1];
  EUNET_DASSERT(G >= 0 && G <= V && V <= L);
  int carry = block_count[(long long)seg * nb + blockIdx.x];
  double acc = 0.0;
  for (int r = 0; r < LZ_ITEMS; ++r) {  // not unrolled: block_exclusive_scan_flag holds barriers
    const long long i = (long long)blockIdx.x * LZ_T + r * LM_NT + tid;
    const bool in = i < L, valid = i < V;
    const uint32_t pw = in ? pay[so + i] : 0u;
    const bool fg = valid && (pw & 1u);
    int tot;
    const int before = block_exclusive_scan_flag(fg, &tot);
    if (in) {
      const long long idx = pw >> 1;
      EUNET_DASSERT(idx < L);
      if (order) order[so + i] = (int32_t)idx;
      float g = 0.f;
      if (valid) {
        if (G == 0) {
          g = i == 0 ? 1.f : 0.f;
        } else {
          const long long F = (long long)carry + before + (fg ? 1 : 0);
          const long long I = G - F, U = G + (i + 1) - F;
          EUNET_DASSERT(F <= G && U >= 1 && (fg || U >= 2));
          g = fg ? (float)(1.0 / (double)U) : (float)((double)I / ((double)(U - 1) * (double)U));
        }
        const float e = error_of(keys[so + i]);
        const float eb = hinge ? (e < 0.f ? 0.f : e) : e;
        acc += (double)eb * (double)g;
      }
      long long o = so + idx;
      if (by_class) {
        const long long n = idx / HW;
        o = (n * K + seg) * HW + (idx - n * HW);
      }
      if (idx < L) weights[o] = g;  // a store is never issued outside the segment
    }
    carry += tot;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o, 64);
  if ((tid & 63) == 0) red[tid >> 6] = acc;
  __syncthreads();
  if (tid == 0) part[(long long)seg * nb + blockIdx.x] = ((red[0] + red[1]) + red[2]) + red[3];
}

// counts [S][2] int64 from the device words
__global__ void lz_counts_kernel(const int* cnt, int S, int64_t* counts) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < 2 * S) counts[i] = cnt[i];
}

// One block of 256: per segment the fp64 sum of its partials (threads stride over them, a fixed-order LDS tree, as
// pl_sample_sum), then thread 0 selects, averages and fills factor [S], parts [S], loss, counts and bad.
// mode: 0 present (G > 0), 1 all (V > 0), 2 the classes of class_mask with V > 0.
__global__ __launch_bounds__(256) void lz_finalize_kernel(const double* part, int nb, int S, int K, int N,
                                                          int per_image, int mode, int class_mask, const int* cnt,
                                                          const int* nbad, float* factor, float* loss, float* parts,
                                                          int64_t* counts, float* bad) {
  __shared__ double red[256];
  __shared__ double lsum[LZ_MAX_SEG];
  const int tid = threadIdx.x;
  EUNET_DASSERT(S <= LZ_MAX_SEG);
  for (int s = 0; s < S; ++s) {
    double v = 0.0;
    for (int t = tid; t < nb; t += 256) v += part[(long long)s * nb + t];
    red[tid] = v;
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
      if (tid < off) red[tid] += red[tid + off];
      __syncthreads();
    }
    if (tid == 0) lsum[s] = red[0];
    __syncthreads();
  }
  if (tid != 0) return;
  const int groups = per_image ? N : 1, per = S / groups;  // per = K
  double total = 0.0;
  for (int gi = 0; gi < groups; ++gi) {
    int nsel = 0;
    double sum = 0.0;
    for (int j = 0; j < per; ++j) {
      const int s = gi * per + j, c = s % K;
      const int G = cnt[s * 2], V = cnt[s * 2 + 1];
      const bool sel = mode == 0 ? G > 0 : (V > 0 && (mode == 1 || ((class_mask >> c) & 1)));
      if (sel) {
        ++nsel;
        sum += lsum[s];
      }
      if (parts) parts[s] = sel ? (float)lsum[s] : __uint_as_float(0x7FC00000u);
      factor[s] = sel ? 1.f : 0.f;
      if (counts) counts[s * 2] = G, counts[s * 2 + 1] = V;
    }
    const double share = nsel ? 1.0 / ((double)nsel * (double)groups) : 0.0;
    for (int j = 0; j < per; ++j) factor[gi * per + j] *= (float)share;
    total += nsel ? sum / (double)nsel : 0.0;
  }
  loss[0] = (float)(total / (double)groups);
  if (bad) bad[0] = (float)nbad[0];
}

// ---------------------------------------------------------------------------
// backward: w_c = weights factor[segment]
// ---------------------------------------------------------------------------
template <int K, bool HINGE>
__device__ __forceinline__ void bwd_px(const float (&x)[K], int64_t traw, const float (&w)[K], float g0,
                                       float (&g)[K]) {
  if (HINGE) {
#pragma unroll
    for (int c = 0; c < K; ++c) {
      const bool fg = K == 1 ? traw >= 1 : traw == (int64_t)c;
      const float sg = fg ? 1.f : -1.f;
      const float e = 1.f - x[c] * sg;
      g[c] = e > 0.f ? -(g0 * w[c]) * sg : 0.f;
    }
  } else {
    float p[K], a[K];
    softmax_px<K>(x, p);
    float dot = 0.f;
#pragma unroll
    for (int c = 0; c < K; ++c) {
      const float d = p[c] - (traw == (int64_t)c ? 1.f : 0.f);
      a[c] = d > 0.f ? w[c] : (d < 0.f ? -w[c] : 0.f);
      dot += a[c] * p[c];
    }
#pragma unroll
    for (int c = 0; c < K; ++c) g[c] = g0 * (p[c] * (a[c] - dot));
  }
}

template <int K, bool HINGE, bool VEC>
__global__ __launch_bounds__(PL_NT) void lz_bwd_kernel(const float* logits, const int64_t* target, int N, int HW,
                                                       int per_image, const float* weights, const float* factor,
                                                       const float* gloss, float* glog) {
  constexpr int PER = VEC ? 4 : 1;
  long long id;
  int n, p;
  if (!pl_bwd_split<PER>(N, HW, id, n, p)) return;
  float f[K];
#pragma unroll
  for (int c = 0; c < K; ++c) f[c] = factor[per_image ? n * K + c : c];
  const float g0 = gloss[0];
  const long long o = (long long)n * K * HW + p;
  if (VEC) {
    f32x4 xv[K], wv[K], gv[K];
    int64_t tr[4];
    pl_load4<K>(logits + o, HW, xv);
    pl_load4<K>(weights + o, HW, wv);
    pl_load4(target + id, tr);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      float x[K], w[K], g[K];
      pl_px<K>(xv, j, x);
      pl_px<K>(wv, j, w);
#pragma unroll
      for (int c = 0; c < K; ++c) w[c] *= f[c];
      bwd_px<K, HINGE>(x, tr[j], w, g0, g);
#pragma unroll
      for (int c = 0; c < K; ++c) gv[c][j] = g[c];
    }
    pl_store4<K>(glog + o, HW, gv);
  } else {
    float x[K], w[K], g[K];
    pl_load<K>(logits + o, HW, x);
    pl_load<K>(weights + o, HW, w);
#pragma unroll
    for (int c = 0; c < K; ++c) w[c] *= f[c];
    bwd_px<K, HINGE>(x, target[id], w, g0, g);
    pl_store<K>(glog + o, HW, g);
  }
}

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------
// the workspace of a call over S segments of L: keys, payloads, the sort's own, the scan's block counts and segment
// totals, the counters (G, V per segment, then the out-of-range targets), the fp64 partials and the count rows
// (crows rows of up to 5 words: one per block of the errors or the keys kernel, whichever has more)
struct LzWs {
  size_t keys, pay, sort, block_count, seg_tot, cnt, part, cpart, total;
};
inline LzWs lz_ws(int s, int l) {
  LzWs w;
  const size_t pairs = lz_align((size_t)s * (size_t)l * 4);
  const size_t nb = (size_t)lz_blocks(l);
  w.keys = 0;
  w.pay = pairs;
  w.sort = 2 * pairs;
  w.block_count = w.sort + sort_ws(s, l).total;
  w.seg_tot = w.block_count + lz_align((size_t)s * nb * 4);
  w.cnt = w.seg_tot + lz_align((size_t)s * 4);
  w.part = w.cnt + lz_align(((size_t)s * 2 + 2) * 4);
  w.cpart = w.part + lz_align((size_t)s * nb * 8);
  // rows: S nb of the keys kernel; N tiles of the errors kernel, tiles = ceil(HW / 1024) <= 2 ceil(HW / 2048), which
  // is <= 2 S nb per image, and <= L / 1024 + N <= 2 nb + 64 over the batch
  w.total = w.cpart + lz_align(((size_t)s * (2 * nb + 1) + 64) * 5 * 4);
  return w;
}

inline bool lz_seg_ok(int s, long long l) { return s >= 1 && s <= 65535 && l >= 1 && l < (1ll << 31); }

// sorted keys and payloads -> order / weights / part; the counters of ws are already filled
int lz_sort_scan_grad(int S, int L, char* ws, const LzWs& w, int hinge, int by_class, int K, int HW, int32_t* order,
                      float* weights, hipStream_t s, const char* what) {
  uint32_t* keys = (uint32_t*)(ws + w.keys);
  uint32_t* pay = (uint32_t*)(ws + w.pay);
  int* cnt = (int*)(ws + w.cnt);
  int* block_count = (int*)(ws + w.block_count);
  const int rc = lovasz_sort_pairs(keys, pay, S, L, ws + w.sort, s);
  if (rc != EUNET_OK) return rc;
  const int nb = lz_blocks(L);
  const dim3 grid(nb, S);
  lz_fgcount_kernel<<<grid, LM_NT, 0, s>>>(pay, L, nb, cnt, block_count);
  scan_block_counts_kernel<LM_NT><<<S, LM_NT, 0, s>>>(block_count, nb, (int32_t*)(ws + w.seg_tot));
  lz_grad_kernel<<<grid, LM_NT, 0, s>>>(keys, pay, L, nb, cnt, block_count, hinge, by_class, K, HW, order, weights,
                                        (double*)(ws + w.part));
  return eunet::check_launch(what);
}

bool lz_args_ok(int n, int k, int h, int w, int activation, const char* what) {
  if (!pl_shape_ok(n, k, h, w) || (long long)n * h * w >= (1ll << 31)) {
    eunet::set_error("%s: bad shape (" PL_SHAPE_RULE ", N*H*W < 2^31)", what);
    return false;
  }
  if (activation != EUNET_LOVASZ_SOFTMAX && activation != EUNET_LOVASZ_HINGE) {
    eunet::set_error("%s: activation %d is neither EUNET_LOVASZ_SOFTMAX nor EUNET_LOVASZ_HINGE", what, activation);
    return false;
  }
  if (activation == EUNET_LOVASZ_SOFTMAX && k == 1) {
    eunet::set_error("%s: a softmax over K = 1 is constant; use EUNET_LOVASZ_HINGE", what);
    return false;
  }
  return true;
}

template <class... A>
void launch_errors(int k, bool hinge, dim3 grid, hipStream_t s, A... args) {
  by_k(k, [&](auto kc) {
    by_flag(hinge, [&](auto hc) {
      lz_errors_kernel<decltype(kc)::value, decltype(hc)::value><<<grid, PL_NT, 0, s>>>(args...);
    });
  });
}

}  // namespace

extern "C" {

int eunet_lovasz_workspace_bytes(int s, int l, size_t* bytes) {
  EUNET_REQUIRE(bytes && lz_seg_ok(s, l), "lovasz_workspace_bytes: bad args (S 1..65535, L 1..2^31-1)");
  *bytes = lz_ws(s, l).total;
  return EUNET_OK;
}

int eunet_lovasz_errors(const float* logits, const int64_t* target, int n, int k, int h, int w, int activation,
                        int ignore_index, float* errors, uint8_t* flags, void* stream) {
  EUNET_REQUIRE(logits && target && errors && flags, "lovasz_errors: null argument");
  if (!lz_args_ok(n, k, h, w, activation, "lovasz_errors")) return EUNET_ERR_INVALID;
  const int HW = h * w;
  launch_errors(k, activation == EUNET_LOVASZ_HINGE, dim3(pl_tiles(HW), n), (hipStream_t)stream, logits, target, n,
                HW, 0, ignore_index, errors, flags, (uint32_t*)nullptr, (uint32_t*)nullptr, (int*)nullptr);
  return eunet::check_launch("lovasz_errors");
}

int eunet_lovasz_sort(const float* errors, const uint8_t* flags, int s, int l, int32_t* order, float* grad,
                      int64_t* counts, void* ws, void* stream) {
  EUNET_REQUIRE(errors && flags && order && grad && counts && ws && lz_seg_ok(s, l),
                "lovasz_sort: bad args (S 1..65535, L 1..2^31-1)");
  const LzWs w = lz_ws(s, l);
  char* base = (char*)ws;
  hipStream_t st = (hipStream_t)stream;
  int* cnt = (int*)(base + w.cnt);
  int* cpart = (int*)(base + w.cpart);
  const int nb = lz_blocks(l);
  lz_keys_kernel<<<dim3(nb, s), LM_NT, 0, st>>>(errors, flags, l, (uint32_t*)(base + w.keys),
                                                (uint32_t*)(base + w.pay), cpart);
  lz_count_kernel<<<s + 1, LM_NT, 0, st>>>(cpart, s, nb, 3, 1, s, cnt);
  const int rc = lz_sort_scan_grad(s, l, base, w, 0, 0, 1, l, order, grad, st, "lovasz_sort");
  if (rc != EUNET_OK) return rc;
  lz_counts_kernel<<<cdiv(2 * s, 256), 256, 0, st>>>(cnt, s, counts);
  return eunet::check_launch("lovasz_sort");
}

int eunet_lovasz_fwd(const float* logits, const int64_t* target, int n, int k, int h, int w, int activation,
                     int per_image, int classes_mode, int class_mask, int ignore_index, float* weights,
                     float* factor, float* loss, float* parts, int64_t* counts, float* bad, void* ws, void* stream) {
  EUNET_REQUIRE(logits && target && weights && factor && loss && ws, "lovasz_fwd: null argument");
  if (!lz_args_ok(n, k, h, w, activation, "lovasz_fwd")) return EUNET_ERR_INVALID;
  EUNET_REQUIRE(classes_mode >= EUNET_LOVASZ_PRESENT && classes_mode <= EUNET_LOVASZ_LISTED,
                "lovasz_fwd: classes_mode %d", classes_mode);
  EUNET_REQUIRE(classes_mode != EUNET_LOVASZ_LISTED || (class_mask > 0 && class_mask < (1 << k)),
                "lovasz_fwd: class_mask %d names no class of 0..%d, or one beyond", class_mask, k - 1);
  const int HW = h * w;
  const int S = per_image ? n * k : k, L = per_image ? HW : n * HW;
  const bool hinge = activation == EUNET_LOVASZ_HINGE;
  const LzWs lw = lz_ws(S, L);
  char* base = (char*)ws;
  hipStream_t st = (hipStream_t)stream;
  int* cnt = (int*)(base + lw.cnt);
  int* cpart = (int*)(base + lw.cpart);
  const int tiles = pl_tiles(HW);
  launch_errors(k, hinge, dim3(tiles, n), st, logits, target, n, HW, per_image ? 1 : 0, ignore_index,
                (float*)nullptr, (uint8_t*)nullptr, (uint32_t*)(base + lw.keys), (uint32_t*)(base + lw.pay), cpart);
  lz_count_kernel<<<S + 1, LM_NT, 0, st>>>(cpart, per_image ? n : 1, per_image ? tiles : n * tiles, k + 2, k, S, cnt);
  const int rc = lz_sort_scan_grad(S, L, base, lw, hinge ? 1 : 0, per_image ? 0 : 1, k, HW, nullptr, weights, st,
                                   "lovasz_fwd");
  if (rc != EUNET_OK) return rc;
  lz_finalize_kernel<<<1, 256, 0, st>>>((const double*)(base + lw.part), lz_blocks(L), S, k, n, per_image ? 1 : 0,
                                        classes_mode, class_mask, cnt, cnt + 2 * S, factor, loss, parts, counts, bad);
  return eunet::check_launch("lovasz_fwd");
}

int eunet_lovasz_bwd(const float* logits, const int64_t* target, int n, int k, int h, int w, int activation,
                     int per_image, const float* weights, const float* factor, const float* gloss, float* glogits,
                     void* stream) {
  EUNET_REQUIRE(logits && target && weights && factor && gloss && glogits, "lovasz_bwd: null argument");
  if (!lz_args_ok(n, k, h, w, activation, "lovasz_bwd")) return EUNET_ERR_INVALID;
  const int HW = h * w;
  const bool vec = pl_vec_ok(HW, {logits, target, weights, glogits});
  hipStream_t s = (hipStream_t)stream;
  by_k(k, [&](auto kc) {
    by_flag(activation == EUNET_LOVASZ_HINGE, [&](auto hc) {
      by_flag(vec, [&](auto vc) {
        lz_bwd_kernel<decltype(kc)::value, decltype(hc)::value, decltype(vc)::value>
            <<<pl_bwd_grid(n, HW, vec), PL_NT, 0, s>>>(logits, target, n, HW, per_image ? 1 : 0, weights, factor,
                                                       gloss, glogits);
      });
    });
  });
  return eunet::check_launch("lovasz_bwd");
}

}  // extern "C"
