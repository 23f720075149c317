// Instance-level evaluation: pairwise mask overlap, binary morphology, connected-component
// labelling, outer-border following and the per-pixel helpers of the instance split.
//
// Reference: metrics.py:61-194 (calculate_instance_metrics: calculate_iou per (prediction,
// ground-truth) pair), train_eval.py:654-850 (semantic_to_instances: cv2.morphologyEx / erode /
// dilate, skimage.measure.label(connectivity=2), cv2.findContours + arcLength).
// All of it is integer work: bit-exact, order-free (integer atomics), no floating point.
#include "common.h"
#include "labelmap.h"

EUNET_DEBUG_UNIT(instances)

namespace {

constexpr int NT = 256;
static_assert(NT == LM_NT, "labelmap.h sizes and scans blocks of NT");
constexpr int GRID_CAP = 8192;  // blocks of a grid-stride launch

// ---- bit-pack: masks [n][hw] uint8 (non-zero = set) -> packed [n][words] uint64, words = ceil(hw/64);
// one wave64 ballot = one word; pixels past hw read as clear (zero-filled tail word); areas[n] += popcount
__global__ __launch_bounds__(NT) void pack_masks_kernel(const uint8_t* masks, long long hw, long long words,
                                                        unsigned long long* packed, unsigned long long* areas) {
  const int n = blockIdx.y;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const uint8_t* m = masks + (long long)n * hw;
  unsigned long long* out = packed + (long long)n * words;
  unsigned int area = 0;  // hw < 2^31
  for (long long j = (long long)blockIdx.x * (NT / 64) + wv; j < words; j += (long long)gridDim.x * (NT / 64)) {
    const long long px = j * 64 + lane;
    const bool set = px < hw && m[px] != 0;
    const unsigned long long word = __ballot(set);
    if (lane == 0) {
      EUNET_DASSERT(j >= 0 && j < words);
      out[j] = word;
      area += (unsigned)__popcll(word);
    }
  }
  if (lane == 0 && area) atomicAdd(areas + n, (unsigned long long)area);
}

// ---- the same pass with the bounding box of the set pixels (cv2.boundingRect, train_eval.py:959, 978):
// bbox[n] = (xmin, ymin, xmax, ymax), inclusive, preset to (w, h, -1, -1) by bbox_init_kernel.  A 64-pixel
// word crosses image rows whenever w % 64 != 0, so x and y are derived per lane; min / max are reduced in
// the wave (shuffles), in the block (LDS), then by integer atomicMin / atomicMax (order-free).
__global__ __launch_bounds__(NT) void bbox_init_kernel(int* bbox, int n, int h, int w) {
  const int k = blockIdx.x * NT + threadIdx.x;
  if (k >= n) return;
  bbox[4 * k + 0] = w; bbox[4 * k + 1] = h; bbox[4 * k + 2] = -1; bbox[4 * k + 3] = -1;
}

__global__ __launch_bounds__(NT) void pack_masks_bbox_kernel(const uint8_t* masks, long long hw, int h, int w,
                                                             long long words, unsigned long long* packed,
                                                             unsigned long long* areas, int* bbox) {
  __shared__ int red[NT / 64][4];
  const int n = blockIdx.y;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const uint8_t* m = masks + (long long)n * hw;
  unsigned long long* out = packed + (long long)n * words;
  unsigned int area = 0;  // hw < 2^31
  int xmin = w, ymin = h, xmax = -1, ymax = -1;
  for (long long j = (long long)blockIdx.x * (NT / 64) + wv; j < words; j += (long long)gridDim.x * (NT / 64)) {
    const long long px = j * 64 + lane;
    const bool set = px < hw && m[px] != 0;
    const unsigned long long word = __ballot(set);
    if (set) {
      const int y = (int)((unsigned)px / (unsigned)w), x = (int)((unsigned)px - (unsigned)y * (unsigned)w);
      EUNET_DASSERT(x >= 0 && x < w && y >= 0 && y < h);
      xmin = min(xmin, x); ymin = min(ymin, y);
      xmax = max(xmax, x); ymax = max(ymax, y);
    }
    if (lane == 0) {
      EUNET_DASSERT(j >= 0 && j < words);
      out[j] = word;
      area += (unsigned)__popcll(word);
    }
  }
  if (lane == 0 && area) atomicAdd(areas + n, (unsigned long long)area);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    xmin = min(xmin, __shfl_xor(xmin, o, 64)); ymin = min(ymin, __shfl_xor(ymin, o, 64));
    xmax = max(xmax, __shfl_xor(xmax, o, 64)); ymax = max(ymax, __shfl_xor(ymax, o, 64));
  }
  if (lane == 0) {
    red[wv][0] = xmin; red[wv][1] = ymin; red[wv][2] = xmax; red[wv][3] = ymax;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int i = 1; i < NT / 64; ++i) {
      xmin = min(xmin, red[i][0]); ymin = min(ymin, red[i][1]);
      xmax = max(xmax, red[i][2]); ymax = max(ymax, red[i][3]);
    }
    if (xmax >= 0) {  // this block saw a set pixel
      int* b = bbox + 4ll * n;
      atomicMin(b + 0, xmin); atomicMin(b + 1, ymin);
      atomicMax(b + 2, xmax); atomicMax(b + 3, ymax);
    }
  }
}

// ---- COCOeval.evaluateImg's greedy matching of one image (pycocotools cocoeval.py), every class, both IoU
// types and every threshold in one launch: one block per (class, threshold, type).  The block walks its
// class's detections in the order given (the host sorted them); for each, the lanes stride over the ground
// truths of the class and reduce to the untaken one with the largest IoU >= min(thr, 1 - 1e-10), the LARGER
// index on equal IoU (pycocotools skips on `<`, so a later equal ground truth overwrites an earlier one).
// Taken flags live in an LDS bitset.  IoU is int / int in fp64 (a correctly rounded divide: bit-equal to
// the host's).  Every loop is bounded by D or G; blocks are independent of one another.
constexpr int CM_MAX_D = 4096, CM_MAX_G = 8192, CM_MAX_T = 16;
struct CocoThrs {
  double v[CM_MAX_T];
};

__device__ __forceinline__ double coco_bbox_iou(int4 a, int4 b) {  // (x, y, w, h)
  const int iw = min(a.x + a.z, b.x + b.z) - max(a.x, b.x);
  const int ih = min(a.y + a.w, b.y + b.w) - max(a.y, b.y);
  if (iw <= 0 || ih <= 0) return 0.0;
  const long long i = (long long)iw * ih;
  const long long u = (long long)a.z * a.w + (long long)b.z * b.w - i;
  return (double)i / (double)u;
}

__global__ __launch_bounds__(NT) void coco_match_kernel(const long long* inter, const long long* area_d,
                                                        const long long* area_g, const int4* box_d,
                                                        const int4* box_g, const int* cls_d, const int* cls_g, int D,
                                                        int G, CocoThrs thrs, int T, int* match) {
  __shared__ unsigned taken[CM_MAX_G / 32];
  __shared__ double w_iou[NT / 64];
  __shared__ int w_g[NT / 64];
  const int c = blockIdx.x, t = blockIdx.y, type = blockIdx.z;
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  for (int i = threadIdx.x; i < CM_MAX_G / 32; i += NT) taken[i] = 0u;
  __syncthreads();
  const double thr = fmin(thrs.v[t], 1.0 - 1e-10);
  int* out = match + ((long long)type * T + t) * D;
  for (int d = 0; d < D; ++d) {
    if (cls_d[d] != c) continue;  // block-uniform
    const long long* row = inter + (long long)d * G;
    const long long ad = area_d[d];
    const int4 bd = box_d[d];
    double best = -1.0;
    int bg = -1;
    for (int g = threadIdx.x; g < G; g += NT) {
      if (cls_g[g] != c || ((taken[g >> 5] >> (g & 31)) & 1u)) continue;
      double iou;
      if (type == 0) {
        iou = coco_bbox_iou(bd, box_g[g]);
      } else {
        const long long it = row[g];
        iou = it == 0 ? 0.0 : (double)it / (double)(ad + area_g[g] - it);
      }
      if (iou >= thr && iou >= best) {  // g grows within a lane: >= keeps the later of equals
        best = iou;
        bg = g;
      }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const double oi = __shfl_xor(best, o, 64);
      const int og = __shfl_xor(bg, o, 64);
      if (oi > best || (oi == best && og > bg)) {
        best = oi;
        bg = og;
      }
    }
    if (lane == 0) {
      w_iou[wv] = best;
      w_g[wv] = bg;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
      for (int i = 1; i < NT / 64; ++i)
        if (w_iou[i] > best || (w_iou[i] == best && w_g[i] > bg)) {
          best = w_iou[i];
          bg = w_g[i];
        }
      EUNET_DASSERT(bg >= -1 && bg < G);
      if (bg >= 0) taken[bg >> 5] |= 1u << (bg & 31);
      out[d] = bg;
    }
    __syncthreads();
  }
}

// ---- pairwise overlap: inter[p][g] += sum over words of popcount(a[p][k] & b[g][k]); a small "GEMM".
// A block owns a 64 x 64 tile of pairs and one slice of the word dimension (blockIdx.z); it stages KC words
// of 64 + 64 rows in LDS (k-major, so a wave reads consecutive rows) and each lane keeps a 4 x 4 register
// tile (rows ty + 16 i, columns tx + 16 j).  Slices combine with integer atomics (exact, order-free).
constexpr int PT = 64, KC = 16;

__global__ __launch_bounds__(NT) void pairwise_overlap_kernel(const unsigned long long* a, int P,
                                                              const unsigned long long* b, int G, long long words,
                                                              long long chunks_per_split,
                                                              unsigned long long* inter) {
  __shared__ unsigned long long As[KC][PT + 1], Bs[KC][PT + 1];
  const int p0 = blockIdx.y * PT, g0 = blockIdx.x * PT;
  const int tx = threadIdx.x & 15, ty = threadIdx.x >> 4;
  const int lrow = threadIdx.x >> 2, lk = (threadIdx.x & 3) * 4;  // staging: 4 consecutive words of one row
  const long long k_begin = (long long)blockIdx.z * chunks_per_split * KC;
  long long k_end = k_begin + chunks_per_split * KC;
  if (k_end > words) k_end = words;
  unsigned int acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = 0;

  for (long long k0 = k_begin; k0 < k_end; k0 += KC) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const long long k = k0 + lk + q;
      const bool kin = k < k_end;
      const int pr = p0 + lrow, gr = g0 + lrow;
      EUNET_DASSERT(!(kin && pr < P) || ((long long)pr * words + k < (long long)P * words));
      EUNET_DASSERT(!(kin && gr < G) || ((long long)gr * words + k < (long long)G * words));
      As[lk + q][lrow] = (kin && pr < P) ? a[(long long)pr * words + k] : 0ull;
      Bs[lk + q][lrow] = (kin && gr < G) ? b[(long long)gr * words + k] : 0ull;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < KC; ++k) {
      unsigned long long av[4], bv[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) av[i] = As[k][ty + 16 * i];
#pragma unroll
      for (int j = 0; j < 4; ++j) bv[j] = Bs[k][tx + 16 * j];
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] += (unsigned)__popcll(av[i] & bv[j]);
    }
    __syncthreads();
  }
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int p = p0 + ty + 16 * i, g = g0 + tx + 16 * j;
      if (p < P && g < G && acc[i][j]) atomicAdd(inter + (long long)p * G + g, (unsigned long long)acc[i][j]);
    }
}

// ---- binary morphology, OpenCV conventions (cv2.erode / cv2.dilate, train_eval.py:674-776): the element
// is applied un-reflected, dst(x) = min / max over set (i, j) of src(x + (i, j) - anchor), anchor =
// (kw / 2, kh / 2); pixels outside the image never erode and never dilate (they are skipped).
// The elements are what cv2.getStructuringElement(cv2.MORPH_ELLIPSE, (k, k)) returns for k = 2, 3, 5
// (train_eval.py:673, 699, 767), one bit per cell, row-major.
struct MorphElem {
  int k;
  unsigned bits;
};
constexpr unsigned row_bits(int r0, int r1, int r2, int r3, int r4, int k) {
  return (unsigned)r0 | ((unsigned)r1 << k) | ((unsigned)r2 << (2 * k)) | ((unsigned)r3 << (3 * k)) |
         ((unsigned)r4 << (4 * k));
}
// rows are written left-to-right as in numpy; bit j of a row is column j, so the literals are mirrored
const MorphElem MORPH_ELEMS[3] = {
    {2, row_bits(0b10 /*0 1*/, 0b11 /*1 1*/, 0, 0, 0, 2)},
    {3, row_bits(0b010, 0b111, 0b010, 0, 0, 3)},
    {5, row_bits(0b00100, 0b11111, 0b11111, 0b11111, 0b00100, 5)},
};

__global__ __launch_bounds__(NT) void morph_kernel(const uint8_t* src, uint8_t* dst, int h, int w, int k,
                                                   unsigned bits, int dilate) {
  const long long total = (long long)h * w;
  const int anchor = k / 2;
  for (long long id = (long long)blockIdx.x * NT + threadIdx.x; id < total; id += (long long)gridDim.x * NT) {
    const int x = (int)(id % w), y = (int)(id / w);
    unsigned v = dilate ? 0u : 255u;
    for (int i = 0; i < k; ++i) {
      const int yy = y + i - anchor;
      if (yy < 0 || yy >= h) continue;
      for (int j = 0; j < k; ++j) {
        const int xx = x + j - anchor;
        if (!((bits >> (i * k + j)) & 1u) || xx < 0 || xx >= w) continue;
        EUNET_DASSERT((long long)yy * w + xx < total);
        const unsigned s = src[(long long)yy * w + xx];
        v = dilate ? (s > v ? s : v) : (s < v ? s : v);
      }
    }
    dst[id] = (uint8_t)v;
  }
}

// ---- 8-connected component labelling by label equivalence (union-find in global memory).
// parent[i] = i for a set pixel, -1 for a clear one; a union links the larger root under the smaller with
// atomicMin, so parent[i] <= i always holds, parents only decrease, and the root of a finished tree is the
// component's minimum linear index = its first pixel in raster order.  Every loop terminates by that
// monotonicity: find() walks strictly downwards, unite() retries only after a parent has decreased.
// BYVALUE = false: two pixels are equivalent when both are non-zero (scipy.ndimage.label);
// BYVALUE = true: when they hold the same non-zero value (the components of each label of a label map).
template <typename V, bool BYVALUE>
__device__ __forceinline__ bool same_comp(const V* v, long long a, long long b) {
  return BYVALUE ? (v[a] != 0 && v[a] == v[b]) : (v[a] != 0 && v[b] != 0);
}

__device__ __forceinline__ int uf_find(int* parent, int x) {
  int p = __atomic_load_n(parent + x, __ATOMIC_RELAXED);
  while (p != x) {
    EUNET_DASSERT(p >= 0 && p < x);
    x = p;
    p = __atomic_load_n(parent + x, __ATOMIC_RELAXED);
  }
  return x;
}

__device__ __forceinline__ void uf_unite(int* parent, int a, int b) {
  bool done = false;
  while (!done) {
    a = uf_find(parent, a);
    b = uf_find(parent, b);
    if (a == b) {
      done = true;
    } else if (a < b) {
      const int old = atomicMin(parent + b, a);
      done = old == b;
      b = old;
    } else {
      const int old = atomicMin(parent + a, b);
      done = old == a;
      a = old;
    }
  }
}

template <typename V>
__global__ __launch_bounds__(NT) void cc_init_kernel(const V* v, long long total, int* parent) {
  for (long long i = (long long)blockIdx.x * NT + threadIdx.x; i < total; i += (long long)gridDim.x * NT)
    parent[i] = v[i] != 0 ? (int)i : -1;
}

// CONN = 4: W and N only (scipy.ndimage.label's default structure).
template <typename V, bool BYVALUE, int CONN = 8>
__global__ __launch_bounds__(NT) void cc_merge_kernel(const V* v, int h, int w, int* parent) {
  const long long total = (long long)h * w;
  for (long long i = (long long)blockIdx.x * NT + threadIdx.x; i < total; i += (long long)gridDim.x * NT) {
    if (v[i] == 0) continue;
    const int x = (int)(i % w), y = (int)(i / w);
    // the neighbours that precede i in raster order: W, NW, N, NE (W and N when CONN == 4)
    if (x > 0 && same_comp<V, BYVALUE>(v, i, i - 1)) uf_unite(parent, (int)i, (int)(i - 1));
    if (y > 0) {
      const long long up = i - w;
      EUNET_DASSERT(up >= 0 && up + 1 < total);
      if (CONN == 8 && x > 0 && same_comp<V, BYVALUE>(v, i, up - 1)) uf_unite(parent, (int)i, (int)(up - 1));
      if (same_comp<V, BYVALUE>(v, i, up)) uf_unite(parent, (int)i, (int)up);
      if (CONN == 8 && x + 1 < w && same_comp<V, BYVALUE>(v, i, up + 1)) uf_unite(parent, (int)i, (int)(up + 1));
    }
  }
}

__global__ __launch_bounds__(NT) void cc_compress_kernel(long long total, int* parent) {
  for (long long i = (long long)blockIdx.x * NT + threadIdx.x; i < total; i += (long long)gridDim.x * NT)
    if (parent[i] >= 0) parent[i] = uf_find(parent, (int)i);
}

// prefix sum over the root flags (parent[i] == i), in three launches: per-block counts of NT consecutive
// pixels, one block scanning the counts (labelmap.h), per-block ranks.  labels[root] = 1 + number of roots before it.
__global__ __launch_bounds__(NT) void cc_count_roots_kernel(const int* parent, long long total, int* block_count) {
  const long long i = (long long)blockIdx.x * NT + threadIdx.x;
  int tot;
  block_exclusive_scan_flag(i < total && parent[i] == (int)i, &tot);
  if (threadIdx.x == 0) block_count[blockIdx.x] = tot;
}

__global__ __launch_bounds__(NT) void cc_rank_roots_kernel(const int* parent, long long total, const int* block_off,
                                                           int* labels) {
  const long long i = (long long)blockIdx.x * NT + threadIdx.x;
  const bool root = i < total && parent[i] == (int)i;
  int tot;
  const int before = block_exclusive_scan_flag(root, &tot);
  if (root) labels[i] = block_off[blockIdx.x] + before + 1;
}

// labels[i] = labels[root of i] (roots already hold their number and are not written here); areas[label-1] += 1,
// one atomic per wave where the whole wave sits in one component
__global__ __launch_bounds__(NT) void cc_relabel_kernel(const int* parent, long long total, int* labels, int* areas,
                                                        int cap) {
  const long long blocks = (total + NT - 1) / NT;
  for (long long blk = blockIdx.x; blk < blocks; blk += gridDim.x) {
    const long long i = blk * NT + threadIdx.x;
    int lab = 0;
    if (i < total) {
      const int r = parent[i];
      if (r >= 0) {
        EUNET_DASSERT(r <= (int)i && parent[r] == r);
        lab = labels[r];
        if (r != (int)i) labels[i] = lab;
      } else {
        labels[i] = 0;
      }
    }
    EUNET_DASSERT(lab >= 0 && lab <= cap);
    const int first = __shfl(lab, 0, 64);
    const unsigned long long same = __ballot(lab == first);
    if (same == ~0ull) {
      if ((threadIdx.x & 63) == 0 && lab > 0 && lab <= cap) atomicAdd(areas + lab - 1, 64);
    } else if (lab > 0 && lab <= cap) {
      atomicAdd(areas + lab - 1, 1);
    }
  }
}

// ---- per-label statistics of an int32 label map (labels 1..n): stats[k-1] = (n_axis, n_diag, area, start,
// x0, y0, x1, y1).  start = the largest component root of the label = the raster-first pixel of the
// component whose first pixel comes last (contours[0] of cv2.findContours: OpenCV lists the external
// contours in reverse order of discovery).  This choice lives here and nowhere else.
constexpr int ST = 8;

__global__ __launch_bounds__(NT) void label_stats_init_kernel(int* stats, int n, int h, int w) {
  const int k = blockIdx.x * NT + threadIdx.x;
  if (k >= n) return;
  int* s = stats + (long long)k * ST;
  s[0] = 0; s[1] = 0; s[2] = 0; s[3] = -1;
  s[4] = w; s[5] = h; s[6] = -1; s[7] = -1;
}

__global__ __launch_bounds__(NT) void label_stats_kernel(const int* lab, const int* parent, int h, int w, int n,
                                                         int* stats) {
  const long long total = (long long)h * w;
  for (long long i = (long long)blockIdx.x * NT + threadIdx.x; i < total; i += (long long)gridDim.x * NT) {
    const int k = lab[i];
    if (k <= 0 || k > n) continue;
    const int x = (int)(i % w), y = (int)(i / w);
    int* s = stats + (long long)(k - 1) * ST;
    atomicAdd(s + 2, 1);
    if (parent[i] == (int)i) atomicMax(s + 3, (int)i);
    atomicMin(s + 4, x);
    atomicMin(s + 5, y);
    atomicMax(s + 6, x);
    atomicMax(s + 7, y);
  }
}

// Suzuki-Abe outer-border following, 8-connectivity (cv2.findContours(RETR_EXTERNAL), train_eval.py:819),
// one lane per label.  Directions: 0 E, 1 NE, 2 N, 3 NW, 4 W, 5 SW, 6 S, 7 SE (y grows downwards).
// From the start pixel (whose W, NW, N, NE neighbours are clear) search clockwise from W for the first set
// neighbour i1; none: an isolated pixel, (0, 0).  Then walk: from the current pixel scan counter-clockwise
// from the direction after the one pointing back; step; stop when the step arrives at the start from i1.
// Even directions are axis steps, odd ones diagonal.  The walk is capped at 4 * (bounding-box pixels) + 4
// steps, so a logic error ends in a wrong count, never in a kernel that does not return.
__device__ __forceinline__ int dir_dx(int s) { return (int)((0x901Au >> (2 * s)) & 3u) - 1; }  // 1 1 0 -1 -1 -1 0 1
__device__ __forceinline__ int dir_dy(int s) { return (int)((0xA901u >> (2 * s)) & 3u) - 1; }  // 0 -1 -1 -1 0 1 1 1

__global__ __launch_bounds__(64) void outer_border_kernel(const int* lab, int h, int w, int n, int* stats) {
  const int k = blockIdx.x * 64 + threadIdx.x + 1;
  if (k > n) return;
  int* st = stats + (long long)(k - 1) * ST;
  const int start = st[3];
  if (start < 0) return;  // an empty label: (0, 0)
  const int x0 = start % w, y0 = start / w;
  auto at = [&](int x, int y) { return x >= 0 && x < w && y >= 0 && y < h && lab[(long long)y * w + x] == k; };
  EUNET_DASSERT(at(x0, y0));
  const long long bbox = (long long)(st[6] - st[4] + 1) * (st[7] - st[5] + 1);
  const long long cap = 4 * bbox + 4;
  int s = 4;
  const int s_first = 4;
  do {
    s = (s - 1) & 7;
  } while (!at(x0 + dir_dx(s), y0 + dir_dy(s)) && s != s_first);
  if (s == s_first) return;  // isolated pixel
  const int x1 = x0 + dir_dx(s), y1 = y0 + dir_dy(s);
  int x3 = x0, y3 = y0, n_axis = 0, n_diag = 0;
  for (long long step = 0; step < cap; ++step) {
    int t = 1;
    for (; t <= 8; ++t) {
      const int ss = (s + t) & 7;
      if (at(x3 + dir_dx(ss), y3 + dir_dy(ss))) {
        s = ss;
        break;
      }
    }
    EUNET_DASSERT(t <= 8);
    if (t > 8) break;
    const int x4 = x3 + dir_dx(s), y4 = y3 + dir_dy(s);
    if (s & 1) ++n_diag; else ++n_axis;
    if (x4 == x0 && y4 == y0 && x3 == x1 && y3 == y1) break;
    x3 = x4;
    y3 = y4;
    s = (s + 4) & 7;
  }
  st[0] = n_axis;
  st[1] = n_diag;
}

// ---- per-pixel helpers of the split (HBM-bound, one pass each)
// dst = (src == value) as 0 / 1, count += number of ones
template <typename V>
__global__ __launch_bounds__(NT) void mask_eq_kernel(const V* src, long long total, long long value, uint8_t* dst,
                                                     unsigned long long* count) {
  unsigned int c = 0;
  for (long long i = (long long)blockIdx.x * NT + threadIdx.x; i < total; i += (long long)gridDim.x * NT) {
    const bool e = (long long)src[i] == value;
    dst[i] = e ? 1 : 0;
    c += e;
  }
  c = wave_sum(c);
  if ((threadIdx.x & 63) == 0 && c) atomicAdd(count, (unsigned long long)c);
}

// dst = (a != 0 && b != 0) as 0 / 1 (cv2.bitwise_and of 0/1 images), count += number of ones
__global__ __launch_bounds__(NT) void mask_and_kernel(const uint8_t* a, const uint8_t* b, long long total, uint8_t* dst,
                                                      unsigned long long* count) {
  unsigned int c = 0;
  for (long long i = (long long)blockIdx.x * NT + threadIdx.x; i < total; i += (long long)gridDim.x * NT) {
    const bool e = a[i] != 0 && b[i] != 0;
    dst[i] = e ? 1 : 0;
    c += e;
  }
  c = wave_sum(c);
  if ((threadIdx.x & 63) == 0 && c) atomicAdd(count, (unsigned long long)c);
}

// markers[mask != 0] = label   (final_markers[m > 0] = next_label)
__global__ __launch_bounds__(NT) void write_label_kernel(const uint8_t* mask, long long total, int label, int* markers) {
  for (long long i = (long long)blockIdx.x * NT + threadIdx.x; i < total; i += (long long)gridDim.x * NT)
    if (mask[i] != 0) markers[i] = label;
}

// markers[i] = table[labels[i] - 1] where that entry is > 0 (every small region in one pass)
__global__ __launch_bounds__(NT) void relabel_table_kernel(const int* labels, long long total, const int* table, int n,
                                                           int* markers) {
  for (long long i = (long long)blockIdx.x * NT + threadIdx.x; i < total; i += (long long)gridDim.x * NT) {
    const int l = labels[i];
    if (l <= 0) continue;
    EUNET_DASSERT(l <= n);
    if (l > n) continue;
    const int t = table[l - 1];
    if (t > 0) markers[i] = t;
  }
}

// out[slot][i] = 1 where slot = table[labels[i] - 1] >= 0; out [m][total] is zeroed by the caller
__global__ __launch_bounds__(NT) void expand_labels_kernel(const int* labels, long long total, const int* table, int n,
                                                           int m, uint8_t* out) {
  for (long long i = (long long)blockIdx.x * NT + threadIdx.x; i < total; i += (long long)gridDim.x * NT) {
    const int l = labels[i];
    if (l <= 0 || l > n) continue;
    const int slot = table[l - 1];
    if (slot < 0) continue;
    EUNET_DASSERT(slot < m);
    if (slot < m) out[(long long)slot * total + i] = 1;
  }
}

template <typename V, bool BYVALUE, int CONN = 8>
void launch_components(const V* v, int h, int w, int* parent, hipStream_t s) {
  const long long total = (long long)h * w;
  const unsigned g = grid_for(total, GRID_CAP);
  cc_init_kernel<V><<<g, NT, 0, s>>>(v, total, parent);
  cc_merge_kernel<V, BYVALUE, CONN><<<g, NT, 0, s>>>(v, h, w, parent);
  cc_compress_kernel<<<g, NT, 0, s>>>(total, parent);
}

// the labelling behind eunet_label_components (CONN 8) and eunet_label_components_conn; the arguments are checked
template <int CONN>
int label_components_impl(const uint8_t* img, int h, int w, int32_t* labels, int32_t* n_out, int32_t* areas,
                          int areas_cap, int32_t* ws, hipStream_t s, const char* what) {
  const long long total = (long long)h * w;
  if (!fill_async(areas, 0, sizeof(int32_t) * (size_t)areas_cap, s, what)) return EUNET_ERR_HIP;
  int* parent = ws;
  int* block_count = ws + total;
  const long long nb = (total + NT - 1) / NT;
  launch_components<uint8_t, false, CONN>(img, h, w, parent, s);
  cc_count_roots_kernel<<<(unsigned)nb, NT, 0, s>>>(parent, total, block_count);
  scan_block_counts_kernel<NT><<<1, NT, 0, s>>>(block_count, (int)nb, n_out);
  cc_rank_roots_kernel<<<(unsigned)nb, NT, 0, s>>>(parent, total, block_count, labels);
  cc_relabel_kernel<<<grid_for(total, GRID_CAP), NT, 0, s>>>(parent, total, labels, areas, areas_cap);
  EUNET_LAUNCH_CHECK(what);
  return EUNET_OK;
}

}  // namespace

extern "C" {

int eunet_pack_masks(const uint8_t* masks, int n, int h, int w, uint64_t* packed, int64_t* areas, void* stream) {
  EUNET_REQUIRE(masks && packed && areas && n > 0 && h > 0 && w > 0, "pack_masks: bad args");
  const long long hw = (long long)h * w;
  EUNET_REQUIRE(hw < (1ll << 31), "pack_masks: h * w must be below 2^31");
  EUNET_REQUIRE(n <= 65535, "pack_masks: at most 65535 masks per call");
  hipStream_t s = (hipStream_t)stream;
  if (!fill_async(areas, 0, sizeof(int64_t) * n, s, "pack_masks")) return EUNET_ERR_HIP;
  const long long words = (hw + 63) / 64;
  long long bx = (words + NT / 64 - 1) / (NT / 64);
  if (bx > 512) bx = 512;
  pack_masks_kernel<<<dim3((unsigned)bx, n), NT, 0, s>>>(masks, hw, words, (unsigned long long*)packed,
                                                          (unsigned long long*)areas);
  EUNET_LAUNCH_CHECK("pack_masks");
  return EUNET_OK;
}

int eunet_pack_masks_bbox(const uint8_t* masks, int n, int h, int w, uint64_t* packed, int64_t* areas, int32_t* bbox,
                          void* stream) {
  EUNET_REQUIRE(masks && packed && areas && bbox && n > 0 && h > 0 && w > 0, "pack_masks_bbox: bad args");
  const long long hw = (long long)h * w;
  EUNET_REQUIRE(hw < (1ll << 31), "pack_masks_bbox: h * w must be below 2^31");
  EUNET_REQUIRE(n <= 65535, "pack_masks_bbox: at most 65535 masks per call");
  hipStream_t s = (hipStream_t)stream;
  if (!fill_async(areas, 0, sizeof(int64_t) * n, s, "pack_masks_bbox")) return EUNET_ERR_HIP;
  bbox_init_kernel<<<cdiv(n, NT), NT, 0, s>>>(bbox, n, h, w);
  const long long words = (hw + 63) / 64;
  long long bx = (words + NT / 64 - 1) / (NT / 64);
  if (bx > 512) bx = 512;
  pack_masks_bbox_kernel<<<dim3((unsigned)bx, n), NT, 0, s>>>(masks, hw, h, w, words, (unsigned long long*)packed,
                                                               (unsigned long long*)areas, bbox);
  EUNET_LAUNCH_CHECK("pack_masks_bbox");
  return EUNET_OK;
}

int eunet_coco_match(const int64_t* inter, const int64_t* area_d, const int64_t* area_g, const int32_t* box_d,
                     const int32_t* box_g, const int32_t* cls_d, const int32_t* cls_g, int d, int g,
                     const double* thrs, int t, int32_t* match, void* stream) {
  EUNET_REQUIRE(inter && area_d && area_g && box_d && box_g && cls_d && cls_g && thrs && match && d > 0 && g > 0 &&
                    t > 0,
                "coco_match: bad args");
  EUNET_REQUIRE(d <= CM_MAX_D, "coco_match: at most %d detections per image (got %d)", CM_MAX_D, d);
  EUNET_REQUIRE(g <= CM_MAX_G, "coco_match: at most %d ground truths per image (got %d)", CM_MAX_G, g);
  EUNET_REQUIRE(t <= CM_MAX_T, "coco_match: at most %d IoU thresholds (got %d)", CM_MAX_T, t);
  EUNET_REQUIRE((((uintptr_t)box_d | (uintptr_t)box_g) & 15) == 0, "coco_match: boxes must be 16-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  // the classes select the block that writes a detection's row: read them back and check them here
  std::vector<int32_t> cls((size_t)d + g);
  if (hipMemcpyAsync(cls.data(), cls_d, sizeof(int32_t) * d, hipMemcpyDeviceToHost, s) != hipSuccess ||
      hipMemcpyAsync(cls.data() + d, cls_g, sizeof(int32_t) * g, hipMemcpyDeviceToHost, s) != hipSuccess ||
      hipStreamSynchronize(s) != hipSuccess) {
    eunet::set_error("coco_match: reading the classes back failed");
    return EUNET_ERR_HIP;
  }
  for (int32_t c : cls) EUNET_REQUIRE(c == 0 || c == 1, "coco_match: classes must be 0 or 1 (got %d)", (int)c);
  CocoThrs th = {};
  for (int i = 0; i < t; ++i) th.v[i] = thrs[i];
  coco_match_kernel<<<dim3(2, t, 2), NT, 0, s>>>((const long long*)inter, (const long long*)area_d,
                                                 (const long long*)area_g, (const int4*)box_d, (const int4*)box_g,
                                                 cls_d, cls_g, d, g, th, t, match);
  EUNET_LAUNCH_CHECK("coco_match");
  return EUNET_OK;
}

int eunet_pairwise_overlap(const uint64_t* a, int p, const uint64_t* b, int g, long long words, int64_t* inter,
                           void* stream) {
  EUNET_REQUIRE(a && b && inter && p > 0 && g > 0 && words > 0, "pairwise_overlap: bad args");
  EUNET_REQUIRE(words <= (1ll << 25), "pairwise_overlap: h * w must be below 2^31 (words <= 2^25)");
  const int tp = cdiv(p, PT), tg = cdiv(g, PT);
  EUNET_REQUIRE(tp <= 65535, "pairwise_overlap: too many masks");
  hipStream_t s = (hipStream_t)stream;
  if (!fill_async(inter, 0, sizeof(int64_t) * (size_t)p * g, s, "pairwise_overlap")) return EUNET_ERR_HIP;
  // split the word dimension when the pair tiles alone leave most of the 256 CUs idle (~4 blocks per CU)
  const long long chunks = (words + KC - 1) / KC;
  long long splits = 1024 / ((long long)tp * tg);
  if (splits < 1) splits = 1;
  if (splits > chunks) splits = chunks;
  const long long per = (chunks + splits - 1) / splits;
  splits = (chunks + per - 1) / per;  // every slice non-empty
  pairwise_overlap_kernel<<<dim3(tg, tp, (unsigned)splits), NT, 0, s>>>(
      (const unsigned long long*)a, p, (const unsigned long long*)b, g, words, per, (unsigned long long*)inter);
  EUNET_LAUNCH_CHECK("pairwise_overlap");
  return EUNET_OK;
}

int eunet_morph_u8(const uint8_t* src, uint8_t* dst, uint8_t* tmp, int h, int w, int elem, int dilate, int iterations,
                   void* stream) {
  EUNET_REQUIRE(src && dst && h > 0 && w > 0 && elem >= 0 && elem < 3 && iterations >= 1,
                "morph_u8: bad args (elem 0: 2x2, 1: 3x3, 2: 5x5; iterations >= 1)");
  EUNET_REQUIRE(iterations == 1 || (tmp && tmp != dst && tmp != src), "morph_u8: iterations > 1 need a tmp image");
  EUNET_REQUIRE(src != dst, "morph_u8: not in place");
  EUNET_REQUIRE((long long)h * w < (1ll << 31), "morph_u8: h * w must be below 2^31");
  const MorphElem e = MORPH_ELEMS[elem];
  const unsigned g = grid_for((long long)h * w, GRID_CAP);
  const uint8_t* in = src;
  for (int it = 0; it < iterations; ++it) {
    uint8_t* out = ((iterations - 1 - it) & 1) ? tmp : dst;  // the last pass writes dst
    morph_kernel<<<g, NT, 0, (hipStream_t)stream>>>(in, out, h, w, e.k, e.bits, dilate ? 1 : 0);
    in = out;
  }
  EUNET_LAUNCH_CHECK("morph_u8");
  return EUNET_OK;
}

int eunet_label_workspace_bytes(int h, int w, size_t* bytes) {
  EUNET_REQUIRE(bytes && h > 0 && w > 0 && (long long)h * w < (1ll << 31), "label_workspace_bytes: bad args");
  const long long total = (long long)h * w;
  *bytes = sizeof(int32_t) * (size_t)(total + (total + NT - 1) / NT);
  return EUNET_OK;
}

int eunet_label_components(const uint8_t* img, int h, int w, int32_t* labels, int32_t* n_out, int32_t* areas,
                           int areas_cap, int32_t* ws, void* stream) {
  EUNET_REQUIRE(img && labels && n_out && areas && ws && h > 0 && w > 0, "label_components: bad args");
  const long long total = (long long)h * w;
  EUNET_REQUIRE(total < (1ll << 31), "label_components: h * w must be below 2^31");
  // an 8-connected component owns at least one cell of every 2 x 2 block grid it touches
  EUNET_REQUIRE(areas_cap >= (long long)((h + 1) / 2) * ((w + 1) / 2),
                "label_components: areas needs ceil(h/2) * ceil(w/2) entries");
  return label_components_impl<8>(img, h, w, labels, n_out, areas, areas_cap, ws, (hipStream_t)stream,
                                  "label_components");
}

int eunet_label_components_conn(const uint8_t* img, int h, int w, int32_t* labels, int32_t* n_out, int32_t* areas,
                                int areas_cap, int32_t* ws, int connectivity, void* stream) {
  EUNET_REQUIRE(img && labels && n_out && areas && ws && h > 0 && w > 0, "label_components_conn: bad args");
  EUNET_REQUIRE(connectivity == 4 || connectivity == 8, "label_components_conn: connectivity must be 4 or 8 (got %d)",
                connectivity);
  const long long total = (long long)h * w;
  EUNET_REQUIRE(total < (1ll << 31), "label_components_conn: h * w must be below 2^31");
  if (connectivity == 8) {
    EUNET_REQUIRE(areas_cap >= (long long)((h + 1) / 2) * ((w + 1) / 2),
                  "label_components_conn: areas needs ceil(h/2) * ceil(w/2) entries at connectivity 8");
    return label_components_impl<8>(img, h, w, labels, n_out, areas, areas_cap, ws, (hipStream_t)stream,
                                    "label_components_conn");
  }
  // one pixel of each component, no two of them 4-adjacent: at most one colour of a checkerboard
  EUNET_REQUIRE(areas_cap >= (total + 1) / 2,
                "label_components_conn: areas needs ceil(h w / 2) entries at connectivity 4");
  return label_components_impl<4>(img, h, w, labels, n_out, areas, areas_cap, ws, (hipStream_t)stream,
                                  "label_components_conn");
}

int eunet_outer_perimeter(const int32_t* labels, int h, int w, int n, int32_t* stats, int32_t* ws, void* stream) {
  EUNET_REQUIRE(labels && stats && ws && h > 0 && w > 0 && n > 0, "outer_perimeter: bad args");
  const long long total = (long long)h * w;
  EUNET_REQUIRE(total < (1ll << 31), "outer_perimeter: h * w must be below 2^31");
  hipStream_t s = (hipStream_t)stream;
  launch_components<int32_t, true>(labels, h, w, ws, s);
  label_stats_init_kernel<<<cdiv(n, NT), NT, 0, s>>>(stats, n, h, w);
  label_stats_kernel<<<grid_for(total, GRID_CAP), NT, 0, s>>>(labels, ws, h, w, n, stats);
  outer_border_kernel<<<cdiv(n, 64), 64, 0, s>>>(labels, h, w, n, stats);
  EUNET_LAUNCH_CHECK("outer_perimeter");
  return EUNET_OK;
}

int eunet_mask_eq(const void* src, int elem_bytes, long long n, long long value, uint8_t* dst, int64_t* count,
                  void* stream) {
  EUNET_REQUIRE(src && dst && count && n > 0 && (elem_bytes == 4 || elem_bytes == 8),
                "mask_eq: bad args (int32 or int64 source)");
  hipStream_t s = (hipStream_t)stream;
  if (!fill_async(count, 0, sizeof(int64_t), s, "mask_eq")) return EUNET_ERR_HIP;
  if (elem_bytes == 8)
    mask_eq_kernel<int64_t><<<grid_for(n, 1024), NT, 0, s>>>((const int64_t*)src, n, value, dst,
                                                             (unsigned long long*)count);
  else
    mask_eq_kernel<int32_t><<<grid_for(n, 1024), NT, 0, s>>>((const int32_t*)src, n, value, dst,
                                                             (unsigned long long*)count);
  EUNET_LAUNCH_CHECK("mask_eq");
  return EUNET_OK;
}

int eunet_mask_and(const uint8_t* a, const uint8_t* b, long long n, uint8_t* dst, int64_t* count, void* stream) {
  EUNET_REQUIRE(a && b && dst && count && n > 0, "mask_and: bad args");
  hipStream_t s = (hipStream_t)stream;
  if (!fill_async(count, 0, sizeof(int64_t), s, "mask_and")) return EUNET_ERR_HIP;
  mask_and_kernel<<<grid_for(n, 1024), NT, 0, s>>>(a, b, n, dst, (unsigned long long*)count);
  EUNET_LAUNCH_CHECK("mask_and");
  return EUNET_OK;
}

int eunet_write_label(const uint8_t* mask, long long n, int label, int32_t* markers, void* stream) {
  EUNET_REQUIRE(mask && markers && n > 0 && label > 0, "write_label: bad args");
  write_label_kernel<<<grid_for(n, GRID_CAP), NT, 0, (hipStream_t)stream>>>(mask, n, label, markers);
  EUNET_LAUNCH_CHECK("write_label");
  return EUNET_OK;
}

int eunet_relabel_table(const int32_t* labels, long long n, const int32_t* table, int n_labels, int32_t* markers,
                        void* stream) {
  EUNET_REQUIRE(labels && table && markers && n > 0 && n_labels > 0, "relabel_table: bad args");
  relabel_table_kernel<<<grid_for(n, GRID_CAP), NT, 0, (hipStream_t)stream>>>(labels, n, table, n_labels, markers);
  EUNET_LAUNCH_CHECK("relabel_table");
  return EUNET_OK;
}

int eunet_expand_labels(const int32_t* labels, long long n, const int32_t* table, int n_labels, int m, uint8_t* out,
                        void* stream) {
  EUNET_REQUIRE(labels && table && out && n > 0 && n_labels > 0 && m > 0, "expand_labels: bad args");
  hipStream_t s = (hipStream_t)stream;
  if (!fill_async(out, 0, (size_t)m * (size_t)n, s, "expand_labels")) return EUNET_ERR_HIP;
  expand_labels_kernel<<<grid_for(n, GRID_CAP), NT, 0, s>>>(labels, n, table, n_labels, m, out);
  EUNET_LAUNCH_CHECK("expand_labels");
  return EUNET_OK;
}

}  // extern "C"
