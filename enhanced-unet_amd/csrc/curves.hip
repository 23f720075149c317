// Pixel-level score histograms: the one pass behind the ROC, PR and calibration statistics.
//
// Reference: train_eval.py:1291-1306 (the per-image softmax copied to the host) and
// visualization.py:1096-1199, 1819-1900 (plot_roc_curves / plot_pr_curves / plot_calibration_curve, which
// sort every pixel's score).  Here one read of the probabilities and of the mask gives, per class and per
// score bin, the number of negatives, the number of positives and a fixed-point confidence sum: integers,
// order-free, so the histogram of a whole validation set is the sum of its images' and every curve follows
// from it on the host (eunet/metrics.py).  The contract is in include/eunet.h (eunet_score_hist).
#include "common.h"
#include "labelmap.h"

namespace {

constexpr int NT = 256;
constexpr int MAX_BINS = 3072;      // 20 B of LDS per bin: 61,444 B, inside the 64 KiB a plain launch may ask for
constexpr int PIX_PER_BLOCK = 4096;  // what the launcher aims at per block (four chunks of 4 NT)
constexpr int MAX_BLOCKS = 2048;     // about 8 blocks a CU; beyond it a block takes more pixels
constexpr int MIN_MATES = 8;         // lanes that must share a key before the wave adds for them once

struct Hist {
  unsigned long long* conf;  // [bins]
  unsigned* cnt;             // [bins][2]: neg, pos
  const float* edges;        // [bins + 1] (the closed last bin never reads edges[bins])
};

// the key of one pixel: 2 bin + truth, or -1 for a pixel that counts nowhere
__device__ __forceinline__ int classify(float p, long long m, int c, int k, long long ignore, const float* edges,
                                        int bins, int top, unsigned& q, unsigned& ninv) {
  q = 0;
  if (m == ignore) return -1;
  if (!(p >= 0.f) || p == INFINITY) {  // NaN, -inf, < 0 (-0.0 passes), +inf
    ++ninv;
    return -1;
  }
  // the largest i in [0, bins-1] with edges[i] <= p (edges[0] = 0 <= p): a fixed number of steps
  int lo = 0;
  for (int s = top; s > 0; s >>= 1) {
    const int mid = lo + s;
    if (mid < bins && edges[mid < bins ? mid : bins - 1] <= p) lo = mid;
  }
  q = (unsigned)rintf(fminf(p, 1.f) * 16777216.f);  // exact scaling, round to nearest even; <= 2^24
  const bool pos = k == 1 ? m >= 1 : m == (long long)c;
  return lo * 2 + (pos ? 1 : 0);
}

__device__ __forceinline__ void add_item(const Hist& h, int key, unsigned count, unsigned q) {
  atomicAdd(&h.cnt[key], count);
  if (q) atomicAdd(&h.conf[key >> 1], (unsigned long long)q);
}

// Every lane brings one item of `count` pixels (the same count on every lane; key < 0: none).  Saturated maps
// put the whole wave on one (bin, truth) address: the lanes that share the first pending lane's key are
// counted with a ballot and added once, at most twice in a row (background next to one cell class); what is
// left adds for itself.  Integer adds: exact either way.
// Called by whole waves only (the ballots and shuffles see all 64 lanes).
__device__ __forceinline__ void wave_add(const Hist& h, int key, unsigned count, unsigned q) {
  const int lane = threadIdx.x & 63;
  unsigned long long todo = __ballot(key >= 0);
#pragma unroll 1
  for (int round = 0; round < 2 && todo; ++round) {
    const int lead = __ffsll((long long)todo) - 1;
    const int lk = __shfl(key, lead, 64);
    const bool mate = key == lk;  // lk >= 0, so a lane without an item is never a mate
    const unsigned long long mates = __ballot(mate);
    if (__popcll(mates) < MIN_MATES) break;
    const unsigned long long qs = wave_sum_wide(mate ? q : 0u);  // each <= 2^26: four pixels of at most 2^24
    if (lane == lead) {
      atomicAdd(&h.cnt[lk], count * (unsigned)__popcll(mates));
      if (qs) atomicAdd(&h.conf[lk >> 1], qs);
    }
    if (mate) key = -1;
    todo &= ~mates;
  }
  if (key >= 0) add_item(h, key, count, q);
}

// grid (x, k, n): block (bx, c, i) bins class c of image i over its share of the pixels.
// Per-block counters are uint32: a block takes at most nchunk / gridDim.x + 1 chunks of 4 NT pixels and block 0
// the head and tail, under hw / gridDim.x + 8 NT + 6 pixels; the launcher keeps gridDim.x > hw / 2^31, so no
// counter passes 2^31 + 2054.  The confidence sum is 64-bit in LDS too.
__global__ __launch_bounds__(NT) void score_hist_kernel(const float* probs, const int64_t* mask, int k, long long hw,
                                                        const float* edges_g, int bins, int top, long long ignore,
                                                        unsigned long long* hist, unsigned long long* invalid) {
  extern __shared__ unsigned long long smem[];
  Hist h;
  h.conf = smem;
  unsigned* cnt = (unsigned*)(smem + bins);
  float* edges = (float*)(cnt + 2 * bins);
  h.cnt = cnt;
  h.edges = edges;
  for (int i = threadIdx.x; i < bins; i += NT) {
    smem[i] = 0ull;
    cnt[2 * i] = 0u;
    cnt[2 * i + 1] = 0u;
  }
  for (int i = threadIdx.x; i <= bins; i += NT) edges[i] = edges_g[i];
  __syncthreads();

  const int c = blockIdx.y, img = blockIdx.z;
  const float* p = probs + ((long long)img * k + c) * hw;
  const int64_t* m = mask + (long long)img * hw;
  unsigned ninv = 0;

  // the plane of class c >= 1 starts c hw floats in: up to 3 scalar pixels reach the first 16-byte unit
  long long head = (long long)(((16u - (unsigned)((uintptr_t)p & 15u)) & 15u) >> 2);
  if (head > hw) head = hw;
  const long long nvec = (hw - head) >> 2;
  const long long tail0 = head + 4 * nvec;  // [tail0, hw): up to 3 scalar pixels
  const f32x4* pv = (const f32x4*)(p + head);
  const int64_t* mv = m + head;

  // whole chunks of NT units, so that every wave enters wave_add with all 64 lanes
  const long long nchunk = (nvec + NT - 1) / NT;
  // the next chunk's loads are issued before this chunk's searches (a dependent chain of LDS reads) start
  f32x4 nv = {0.f, 0.f, 0.f, 0.f};
  int64_t nm[4] = {0, 0, 0, 0};
  auto load = [&](long long ch) {
    const long long u = ch * NT + threadIdx.x;
    if (ch < nchunk && u < nvec) {
      nv = pv[u];
#pragma unroll
      for (int j = 0; j < 4; ++j) nm[j] = mv[4 * u + j];
    }
  };
  load(blockIdx.x);
  for (long long ch = blockIdx.x; ch < nchunk; ch += gridDim.x) {
    const long long u = ch * NT + threadIdx.x;
    const f32x4 v = nv;
    const int64_t mu[4] = {nm[0], nm[1], nm[2], nm[3]};
    load(ch + gridDim.x);
    int key[4] = {-1, -1, -1, -1};
    unsigned q[4] = {0u, 0u, 0u, 0u};
    if (u < nvec) {
#pragma unroll
      for (int j = 0; j < 4; ++j) key[j] = classify(v[j], mu[j], c, k, ignore, edges, bins, top, q[j], ninv);
    }
    // four neighbouring pixels mostly share a key: one item per thread then, and the wave sums those
    const bool same = key[0] == key[1] && key[0] == key[2] && key[0] == key[3];
    wave_add(h, same ? key[0] : -1, 4u, q[0] + q[1] + q[2] + q[3]);
    if (!same) {
#pragma unroll
      for (int j = 0; j < 4; ++j)
        if (key[j] >= 0) add_item(h, key[j], 1u, q[j]);
    }
  }
  if (blockIdx.x == 0 && threadIdx.x < 6) {  // head and tail, one pixel per thread
    const int t = threadIdx.x;
    const long long i = t < 3 ? (long long)t : tail0 + (t - 3);
    if (t < 3 ? i < head : i < hw) {
      unsigned q1;
      const int key1 = classify(p[i], m[i], c, k, ignore, edges, bins, top, q1, ninv);
      if (key1 >= 0) add_item(h, key1, 1u, q1);
    }
  }
  __syncthreads();

  unsigned long long* out = hist + (long long)c * bins * 3;
  for (int b = threadIdx.x; b < bins; b += NT) {
    const unsigned neg = cnt[2 * b], pos = cnt[2 * b + 1];
    const unsigned long long cf = smem[b];
    if (neg) atomicAdd(out + 3 * b + 0, (unsigned long long)neg);
    if (pos) atomicAdd(out + 3 * b + 1, (unsigned long long)pos);
    if (cf) atomicAdd(out + 3 * b + 2, cf);
  }
  ninv = wave_sum(ninv);
  if ((threadIdx.x & 63) == 0 && ninv) atomicAdd(invalid, (unsigned long long)ninv);
}

}  // namespace

extern "C" {

int eunet_score_hist(const float* probs, const int64_t* mask, int n, int k, long long hw, const float* edges,
                     int bins, int ignore_index, int64_t* hist, int64_t* invalid, void* stream) {
  EUNET_REQUIRE(probs && mask && edges && hist && invalid, "score_hist: null pointer");
  EUNET_REQUIRE(n >= 1 && n <= 65535 && k >= 1 && k <= 3 && hw >= 1 && bins >= 1 && bins <= MAX_BINS,
                "score_hist: bad args (n 1..65535, k 1..3, hw >= 1, bins 1..%d)", MAX_BINS);
  EUNET_REQUIRE(((uintptr_t)probs & 3u) == 0 && ((uintptr_t)mask & 7u) == 0, "score_hist: misaligned probs / mask");
  // aim at PIX_PER_BLOCK pixels a block and at most MAX_BLOCKS blocks in all (the searches are chains of LDS
  // reads: what hides them is waves per CU; every block also pays its zeroing and its flush); never fewer blocks
  // than keep a block's uint32 counters safe (hw / gx < 2^31, see the kernel)
  long long gx = (hw + PIX_PER_BLOCK - 1) / PIX_PER_BLOCK;
  const long long cap = MAX_BLOCKS / ((long long)n * k) > 0 ? MAX_BLOCKS / ((long long)n * k) : 1;
  if (gx > cap) gx = cap;
  const long long need = (hw >> 31) + 1;
  if (gx < need) gx = need;
  EUNET_REQUIRE(gx <= 0x7fffffffLL, "score_hist: hw too large");
  int top = bins > 1 ? 1 : 0;  // the largest power of two <= bins - 1 (0 for one bin)
  while (2 * top <= bins - 1 && top) top *= 2;
  const size_t lds = (size_t)bins * 20 + 4;
  score_hist_kernel<<<dim3((unsigned)gx, k, n), NT, lds, (hipStream_t)stream>>>(
      probs, mask, k, hw, edges, bins, top, (long long)ignore_index, (unsigned long long*)hist,
      (unsigned long long*)invalid);
  EUNET_LAUNCH_CHECK("score_hist");
  return EUNET_OK;
}

}  // extern "C"
