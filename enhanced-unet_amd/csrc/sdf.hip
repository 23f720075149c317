// Signed distance maps of a label map and the boundary (surface) loss that streams them against the logits.
//
// No reference line to cite: the reference trains with region losses only.  The loss is the boundary loss of
// Kervadec et al., "Boundary loss for highly unbalanced segmentation" (MIDL 2019): the class probability
// integrated against the signed distance map of the ground truth.  The definitions are in include/eunet.h
// (eunet_signed_distance, eunet_boundary_loss_fwd).
//
//   remap_fg_kernel      K = 1 only: the one class is "foreground", target >= 1, which the transform's equality
//                        predicate cannot say; an int64 scratch plane holds [target >= 1 and not ignored]
//   (eunet_edt_sq twice) the exact squared distances to the class (EQ) and to its complement (NE), boundary.hip
//   sdf_combine_kernel   one thread per pixel (4 on the vector path) and all K classes: reads the two int32 planes
//                        and the target, takes the square root in fp64, writes phi once
//   bl_fwd_kernel        one block per (sample, tile of 1024 pixels): sum_c w_c p_c dist_c, reduced in the wave,
//                        one partial per tile; bl_finalize_kernel sums the partials in fp64 in a fixed order
//   bl_bwd_kernel        per pixel, the softmax recomputed; logits and dist read once, the gradient written once
// All of them are HBM-bound streams with 16-byte accesses when H*W is a multiple of 4.
#include <math.h>

#include "common.h"
#include "labelmap.h"

EUNET_DEBUG_UNIT(sdf)

namespace {
constexpr int NT = 256;
constexpr int LPIX = 1024;  // pixels per partial tile: 4 per thread
constexpr int32_t NONE = EUNET_EDT_NONE;

typedef long long i64x2 __attribute__((ext_vector_type(2)));
typedef int i32x4 __attribute__((ext_vector_type(4)));

struct Weights {
  float w[3];
};

__global__ __launch_bounds__(NT) void remap_fg_kernel(const int64_t* target, long long total, long long ign,
                                                      int64_t* out) {
  for (long long id = (long long)blockIdx.x * NT + threadIdx.x; id < total; id += (long long)gridDim.x * NT) {
    const long long t = (long long)target[id];
    out[id] = (t >= 1 && t != ign) ? 1 : 0;
  }
}

// phi of one pixel and class from the two exact squared distances; live: the class and its complement both occur in
// the sample (neither plane is NONE, so no NONE reaches the square root)
template <int K>
__device__ __forceinline__ float phi_of(long long t, int c, bool live, int32_t d_out, int32_t d_in, long long ign,
                                        double clip, double scale) {
  double v = 0.0;
  if (live && t != ign) {
    const bool in = K == 1 ? t >= 1 : t == (long long)c;
    EUNET_DASSERT(in ? (d_in >= 1 && d_in != NONE && d_out == 0) : (d_out >= 1 && d_out != NONE));
    v = in ? 1.0 - sqrt((double)d_in) : sqrt((double)d_out);
  }
  if (clip > 0.0) v = fmin(fmax(v, -clip), clip);
  return (float)(scale * v);
}

// grid (ceil(HW / (NT * PER)), N).  dout / din: int32 [N][K][HW]
template <int K, bool VEC>
__global__ __launch_bounds__(NT) void sdf_combine_kernel(const int32_t* dout, const int32_t* din,
                                                         const int64_t* target, int HW, long long ign, double clip,
                                                         double scale, float* out) {
  constexpr int PER = VEC ? 4 : 1;
  const int n = blockIdx.y;
  const long long p = ((long long)blockIdx.x * NT + threadIdx.x) * PER;
  if (p >= HW) return;
  EUNET_DASSERT(p + PER <= HW);
  const int32_t* po = dout + (long long)n * K * HW;
  const int32_t* pi = din + (long long)n * K * HW;
  const int64_t* tg = target + (long long)n * HW + p;
  float* o = out + (long long)n * K * HW + p;
  bool live[K];  // a sample without a site is NONE everywhere: element 0 tells
#pragma unroll
  for (int c = 0; c < K; ++c) live[c] = po[(long long)c * HW] != NONE && pi[(long long)c * HW] != NONE;
  if (VEC) {
    const i64x2 t01 = *reinterpret_cast<const i64x2*>(tg);
    const i64x2 t23 = *reinterpret_cast<const i64x2*>(tg + 2);
    const long long tr[4] = {t01[0], t01[1], t23[0], t23[1]};
#pragma unroll
    for (int c = 0; c < K; ++c) {
      const i32x4 a = *reinterpret_cast<const i32x4*>(po + (long long)c * HW + p);
      const i32x4 b = *reinterpret_cast<const i32x4*>(pi + (long long)c * HW + p);
      f32x4 v;
#pragma unroll
      for (int j = 0; j < 4; ++j) v[j] = phi_of<K>(tr[j], c, live[c], a[j], b[j], ign, clip, scale);
      *reinterpret_cast<f32x4*>(o + (long long)c * HW) = v;
    }
  } else {
    const long long t = (long long)tg[0];
#pragma unroll
    for (int c = 0; c < K; ++c)
      o[(long long)c * HW] =
          phi_of<K>(t, c, live[c], po[(long long)c * HW + p], pi[(long long)c * HW + p], ign, clip, scale);
  }
}

// ---- boundary loss ----------------------------------------------------------------------------------------
// sig(x), sig(-x) from one exp: no overflow and no cancellation at +-100 (bce_dice.hip's sigmoid_terms)
__device__ __forceinline__ void sigmoid_pair(float x, float& p, float& q) {
  const float e = expf(-fabsf(x));
  const float r = 1.f / (1.f + e);
  const float hi = r, lo = e * r;
  p = x >= 0.f ? hi : lo;
  q = x >= 0.f ? lo : hi;
}

// the max-subtracted softmax of one pixel
template <int K>
__device__ __forceinline__ void softmax_px(const float (&x)[K], float (&p)[K]) {
  float m = x[0];
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
}

// sum_c w_c p_c dist_c of one pixel
template <int K, bool SOFTMAX>
__device__ __forceinline__ float fwd_px(const float (&x)[K], const float (&d)[K], const Weights& cw) {
  float p[K];
  if (SOFTMAX) {
    softmax_px<K>(x, p);
  } else {
#pragma unroll
    for (int c = 0; c < K; ++c) {
      float q;
      sigmoid_pair(x[c], p[c], q);
    }
  }
  float v = 0.f;
#pragma unroll
  for (int c = 0; c < K; ++c) v += cw.w[c] * d[c] * p[c];
  return v;
}

template <int K, bool SOFTMAX, bool VEC>
__global__ __launch_bounds__(NT) void bl_fwd_kernel(const float* logits, const float* dist, int HW, Weights cw,
                                                    float* part) {
  __shared__ float red[4];
  const int n = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const float* lg = logits + (long long)n * K * HW;
  const float* dg = dist + (long long)n * K * HW;
  float acc = 0.f;
  const int p0 = blockIdx.x * LPIX;
  const int p1 = min(HW, p0 + LPIX);
  if (VEC) {  // HW % 4 == 0: every plane and every 4-pixel group starts on 16 bytes
    const int p = p0 + tid * 4;
    if (p < p1) {
      EUNET_DASSERT(p + 3 < HW);
      f32x4 xv[K], dv[K];
#pragma unroll
      for (int c = 0; c < K; ++c) {
        xv[c] = *reinterpret_cast<const f32x4*>(lg + (long long)c * HW + p);
        dv[c] = *reinterpret_cast<const f32x4*>(dg + (long long)c * HW + p);
      }
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        float x[K], d[K];
#pragma unroll
        for (int c = 0; c < K; ++c) {
          x[c] = xv[c][j];
          d[c] = dv[c][j];
        }
        acc += fwd_px<K, SOFTMAX>(x, d, cw);
      }
    }
  } else {
    for (int p = p0 + tid; p < p1; p += NT) {
      EUNET_DASSERT(p < HW);
      float x[K], d[K];
#pragma unroll
      for (int c = 0; c < K; ++c) {
        x[c] = lg[(long long)c * HW + p];
        d[c] = dg[(long long)c * HW + p];
      }
      acc += fwd_px<K, SOFTMAX>(x, d, cw);
    }
  }
  const float s = wave_sum(acc);
  if (lane == 0) red[wv] = s;
  __syncthreads();
  if (tid == 0) part[(long long)n * gridDim.x + blockIdx.x] = red[0] + red[1] + red[2] + red[3];
}

// One 256-thread block: per sample, the threads stride over the tile partials (fp64), a fixed-order LDS tree
// combines them (deterministic); the batch sum is taken in sample order.  den = H W Kw.
__global__ __launch_bounds__(256) void bl_finalize_kernel(const float* part, int tiles, int N, double den,
                                                          float* loss, float* parts) {
  __shared__ double red[256];
  __shared__ double tot[64];
  const int tid = threadIdx.x;
  EUNET_DASSERT(N <= 64);
  for (int n = 0; n < N; ++n) {
    double v = 0.0;
    for (int t = tid; t < tiles; t += 256) v += (double)part[(long long)n * tiles + t];
    red[tid] = v;
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
      if (tid < off) red[tid] += red[tid + off];
      __syncthreads();
    }
    if (tid == 0) {
      tot[n] = red[0];
      if (parts) parts[n] = (float)(red[0] / den);
    }
    __syncthreads();
  }
  if (tid == 0) {
    double s = 0.0;
    for (int i = 0; i < N; ++i) s += tot[i];
    loss[0] = (float)(s / (den * (double)N));
  }
}

// g[j] = d (sum_c w_c p_c dist_c) / d x_j, before the common factor.  Softmax: p_j (a_j - sum_c p_c a_c) with
// a = w dist, written as p_j sum_{c != j} p_c (a_j - a_c) (sum_c p_c = 1): no difference of nearly equal sums is
// taken when one probability saturates.
template <int K, bool SOFTMAX>
__device__ __forceinline__ void bwd_px(const float (&x)[K], const float (&d)[K], const Weights& cw, float (&g)[K]) {
  if (SOFTMAX) {
    float p[K], a[K];
    softmax_px<K>(x, p);
#pragma unroll
    for (int c = 0; c < K; ++c) a[c] = cw.w[c] * d[c];
#pragma unroll
    for (int j = 0; j < K; ++j) {
      float s = 0.f;
#pragma unroll
      for (int c = 0; c < K; ++c)
        if (c != j) s += p[c] * (a[j] - a[c]);
      g[j] = p[j] * s;
    }
  } else {
#pragma unroll
    for (int c = 0; c < K; ++c) {
      float p, q;
      sigmoid_pair(x[c], p, q);
      g[c] = cw.w[c] * d[c] * (p * q);
    }
  }
}

// VEC: one thread per group of 4 pixels (HW % 4 == 0, so a group never straddles two samples).  inv = 1 / (N H W Kw)
template <int K, bool SOFTMAX, bool VEC>
__global__ __launch_bounds__(NT) void bl_bwd_kernel(const float* logits, const float* dist, int N, int HW, Weights cw,
                                                    float inv, const float* gloss, float* glog) {
  constexpr int PER = VEC ? 4 : 1;
  const long long id = ((long long)blockIdx.x * NT + threadIdx.x) * PER;
  const long long total = (long long)N * HW;
  if (id >= total) return;
  EUNET_DASSERT(id + PER <= total);
  const int n = (int)(id / HW);
  const int p = (int)(id - (long long)n * HW);
  EUNET_DASSERT(n < N && p + PER <= HW);
  const float* lg = logits + (long long)n * K * HW + p;
  const float* dg = dist + (long long)n * K * HW + p;
  float* gl = glog + (long long)n * K * HW + p;
  const float g0 = gloss[0] * inv;
  if (VEC) {
    f32x4 xv[K], dv[K], gv[K];
#pragma unroll
    for (int c = 0; c < K; ++c) {
      xv[c] = *reinterpret_cast<const f32x4*>(lg + (long long)c * HW);
      dv[c] = *reinterpret_cast<const f32x4*>(dg + (long long)c * HW);
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      float x[K], d[K], g[K];
#pragma unroll
      for (int c = 0; c < K; ++c) {
        x[c] = xv[c][j];
        d[c] = dv[c][j];
      }
      bwd_px<K, SOFTMAX>(x, d, cw, g);
#pragma unroll
      for (int c = 0; c < K; ++c) gv[c][j] = g0 * g[c];
    }
#pragma unroll
    for (int c = 0; c < K; ++c) *reinterpret_cast<f32x4*>(gl + (long long)c * HW) = gv[c];
  } else {
    float x[K], d[K], g[K];
#pragma unroll
    for (int c = 0; c < K; ++c) {
      x[c] = lg[(long long)c * HW];
      d[c] = dg[(long long)c * HW];
    }
    bwd_px<K, SOFTMAX>(x, d, cw, g);
#pragma unroll
    for (int c = 0; c < K; ++c) gl[(long long)c * HW] = g0 * g[c];
  }
}

// the shared argument rules of the two loss entries; fills cw and Kw
bool loss_args(const char* what, const void* a, const void* b, const void* c, const void* d, int n, int k, int h,
               int w, int activation, const float* class_weight, Weights* cw, int* kw) {
  if (!(a && b && c && d && n > 0 && n <= 64 && k >= 1 && k <= 3 && h > 0 && w > 0 &&
        (long long)h * w < (1ll << 31) - LPIX)) {
    eunet::set_error("%s: bad args (N <= 64, K <= 3)", what);
    return false;
  }
  if (activation != EUNET_BOUNDARY_SOFTMAX && activation != EUNET_BOUNDARY_SIGMOID) {
    eunet::set_error("%s: unknown activation %d", what, activation);
    return false;
  }
  if (activation == EUNET_BOUNDARY_SOFTMAX && k == 1) {
    eunet::set_error("%s: a softmax over K = 1 is constant (use the sigmoid)", what);
    return false;
  }
  *kw = 0;
  for (int i = 0; i < 3; ++i) {
    cw->w[i] = i < k ? (class_weight ? class_weight[i] : 1.f) : 0.f;
    if (!isfinite(cw->w[i])) {
      eunet::set_error("%s: class_weight[%d] is not finite", what, i);
      return false;
    }
    *kw += cw->w[i] != 0.f;
  }
  if (*kw < 1) *kw = 1;
  return true;
}

}  // namespace

extern "C" {

int eunet_signed_distance_workspace_bytes(int n, int k, int h, int w, size_t* bytes) {
  EUNET_REQUIRE(bytes, "signed_distance_workspace_bytes: null pointer");
  EUNET_REQUIRE(plane_stack_ok(n, h, w, false) && k >= 1 && k <= 3,
                "signed_distance_workspace_bytes: bad shape (k 1..3, h and w 1..%d)", EUNET_EDT_MAX_SIDE);
  const size_t hw = (size_t)h * w;
  *bytes = (size_t)2 * n * k * hw * sizeof(int32_t) + (k == 1 ? (size_t)n * hw * sizeof(int64_t) : 0);
  return EUNET_OK;
}

int eunet_signed_distance(const int64_t* target, int n, int k, int h, int w, int ignore_index, float clip,
                          float scale, int32_t* ws, float* out, void* stream) {
  EUNET_REQUIRE(target && ws && out, "signed_distance: null pointer");
  EUNET_REQUIRE(plane_stack_ok(n, h, w, false) && k >= 1 && k <= 3,
                "signed_distance: bad shape (n 1..65535, k 1..3, h and w 1..%d)", EUNET_EDT_MAX_SIDE);
  EUNET_REQUIRE(isfinite(clip) && clip >= 0.f, "signed_distance: clip must be finite and > 0 (0: no clamp)");
  EUNET_REQUIRE(isfinite(scale), "signed_distance: scale must be finite");
  EUNET_REQUIRE(k == 1 || ignore_index < 0 || ignore_index >= k,
                "signed_distance: ignore_index %d is one of the %d classes", ignore_index, k);
  EUNET_REQUIRE(((uintptr_t)target & 7u) == 0 && ((uintptr_t)ws & 7u) == 0 && ((uintptr_t)out & 3u) == 0,
                "signed_distance: misaligned pointer");
  const hipStream_t s = (hipStream_t)stream;
  const int HW = h * w;
  const long long planes = (long long)n * k * HW;
  int32_t* dout = ws;
  int32_t* din = ws + planes;
  const long long ign = (long long)ignore_index;
  const int64_t* sites = target;
  int64_t values[3] = {0, 1, 2};
  if (k == 1) {
    int64_t* fg = (int64_t*)(ws + 2 * planes);
    const long long total = (long long)n * HW;
    const long long b = (total + NT - 1) / NT;
    remap_fg_kernel<<<(unsigned)(b < 2048 ? b : 2048), NT, 0, s>>>(target, total, ign, fg);
    EUNET_LAUNCH_CHECK("signed_distance");
    sites = fg;
    values[0] = 1;
  }
  int rc = eunet_edt_sq(sites, n, h, w, values, k, EUNET_EDT_EQ, dout, stream);
  if (rc != EUNET_OK) return rc;
  rc = eunet_edt_sq(sites, n, h, w, values, k, EUNET_EDT_NE, din, stream);
  if (rc != EUNET_OK) return rc;
  const bool vec = HW % 4 == 0 && ((uintptr_t)target % 16 == 0) && ((uintptr_t)ws % 16 == 0) &&
                   ((uintptr_t)out % 16 == 0);
  const dim3 grid((unsigned)cdiv(HW, NT * (vec ? 4 : 1)), (unsigned)n);
  const double cl = (double)clip, sc = (double)scale;
#define SK(KK)                                                                                          \
  if (vec) sdf_combine_kernel<KK, true><<<grid, NT, 0, s>>>(dout, din, target, HW, ign, cl, sc, out);   \
  else sdf_combine_kernel<KK, false><<<grid, NT, 0, s>>>(dout, din, target, HW, ign, cl, sc, out);
  if (k == 1) { SK(1) } else if (k == 2) { SK(2) } else { SK(3) }
#undef SK
  return eunet::check_launch("signed_distance");
}

int eunet_boundary_loss_workspace_bytes(int n, int h, int w, size_t* bytes) {
  EUNET_REQUIRE(bytes && n > 0 && h > 0 && w > 0, "boundary_loss_workspace_bytes: bad args");
  *bytes = (size_t)n * cdiv(h * w, LPIX) * sizeof(float);
  return EUNET_OK;
}

int eunet_boundary_loss_fwd(const float* logits, const float* dist, int n, int k, int h, int w, int activation,
                            const float* class_weight, float* loss, float* parts, void* ws, void* stream) {
  Weights cw;
  int kw;
  if (!loss_args("boundary_loss_fwd", logits, dist, loss, ws, n, k, h, w, activation, class_weight, &cw, &kw))
    return EUNET_ERR_INVALID;
  const int HW = h * w, tiles = cdiv(HW, LPIX);
  const hipStream_t s = (hipStream_t)stream;
  const dim3 grid(tiles, n);
  const bool vec = HW % 4 == 0 && ((uintptr_t)logits % 16 == 0) && ((uintptr_t)dist % 16 == 0);
  const bool sm = activation == EUNET_BOUNDARY_SOFTMAX;
  float* part = (float*)ws;
#define BK(KK, SS)                                                                           \
  if (vec) bl_fwd_kernel<KK, SS, true><<<grid, NT, 0, s>>>(logits, dist, HW, cw, part);      \
  else bl_fwd_kernel<KK, SS, false><<<grid, NT, 0, s>>>(logits, dist, HW, cw, part);
  if (k == 1) { BK(1, false) }
  else if (k == 2) { if (sm) { BK(2, true) } else { BK(2, false) } }
  else { if (sm) { BK(3, true) } else { BK(3, false) } }
#undef BK
  bl_finalize_kernel<<<1, 256, 0, s>>>(part, tiles, n, (double)HW * kw, loss, parts);
  return eunet::check_launch("boundary_loss_fwd");
}

int eunet_boundary_loss_bwd(const float* logits, const float* dist, int n, int k, int h, int w, int activation,
                            const float* class_weight, const float* gloss, float* glogits, void* stream) {
  Weights cw;
  int kw;
  if (!loss_args("boundary_loss_bwd", logits, dist, gloss, glogits, n, k, h, w, activation, class_weight, &cw, &kw))
    return EUNET_ERR_INVALID;
  const int HW = h * w;
  const bool vec = HW % 4 == 0 && ((uintptr_t)logits % 16 == 0) && ((uintptr_t)dist % 16 == 0) &&
                   ((uintptr_t)glogits % 16 == 0);
  const long long threads = (long long)n * HW / (vec ? 4 : 1);
  const unsigned g = (unsigned)((threads + NT - 1) / NT);
  const hipStream_t s = (hipStream_t)stream;
  const bool sm = activation == EUNET_BOUNDARY_SOFTMAX;
  const float inv = (float)(1.0 / ((double)n * HW * kw));
#define BK(KK, SS)                                                                                      \
  if (vec) bl_bwd_kernel<KK, SS, true><<<g, NT, 0, s>>>(logits, dist, n, HW, cw, inv, gloss, glogits);  \
  else bl_bwd_kernel<KK, SS, false><<<g, NT, 0, s>>>(logits, dist, n, HW, cw, inv, gloss, glogits);
  if (k == 1) { BK(1, false) }
  else if (k == 2) { if (sm) { BK(2, true) } else { BK(2, false) } }
  else { if (sm) { BK(3, true) } else { BK(3, false) } }
#undef BK
  return eunet::check_launch("boundary_loss_bwd");
}

}  // extern "C"
