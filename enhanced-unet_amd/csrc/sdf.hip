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
#include "pixelloss.h"

EUNET_DEBUG_UNIT(sdf)

namespace {
constexpr int32_t NONE = EUNET_EDT_NONE;

typedef long long i64x2 __attribute__((ext_vector_type(2)));
typedef int i32x4 __attribute__((ext_vector_type(4)));

struct Weights {
  float w[3];
};

__global__ __launch_bounds__(PL_NT) void remap_fg_kernel(const int64_t* target, long long total, long long ign,
                                                      int64_t* out) {
  for (long long id = (long long)blockIdx.x * PL_NT + threadIdx.x; id < total; id += (long long)gridDim.x * PL_NT) {
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

// grid (ceil(HW / (PL_NT * PER)), N).  dout / din: int32 [N][K][HW]
template <int K, bool VEC>
__global__ __launch_bounds__(PL_NT) void sdf_combine_kernel(const int32_t* dout, const int32_t* din,
                                                         const int64_t* target, int HW, long long ign, double clip,
                                                         double scale, float* out) {
  constexpr int PER = VEC ? 4 : 1;
  const int n = blockIdx.y;
  const long long p = ((long long)blockIdx.x * PL_NT + threadIdx.x) * PER;
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
// sum_c w_c p_c dist_c of one pixel
template <int K, bool SOFTMAX>
__device__ __forceinline__ float fwd_px(const float (&x)[K], const float (&d)[K], const Weights& cw) {
  float p[K];
  if (SOFTMAX) {
    softmax_px<K>(x, p);
  } else {
#pragma unroll
    for (int c = 0; c < K; ++c) p[c] = sigmoid_terms<false>(x[c]).p;
  }
  float v = 0.f;
#pragma unroll
  for (int c = 0; c < K; ++c) v += cw.w[c] * d[c] * p[c];
  return v;
}

template <int K, bool SOFTMAX, bool VEC>
__global__ __launch_bounds__(PL_NT) void bl_fwd_kernel(const float* logits, const float* dist, int HW, Weights cw,
                                                       float* part) {
  const int n = blockIdx.y;
  const float* lg = logits + (long long)n * K * HW;
  const float* dg = dist + (long long)n * K * HW;
  float acc[1] = {0.f};
  pl_tile_visit<VEC>(HW, [&](int p) {
    float x[K], d[K];
    if constexpr (VEC) {
      f32x4 xv[K], dv[K];
      pl_load4<K>(lg, HW, xv, p);
      pl_load4<K>(dg, HW, dv, p);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        pl_px<K>(xv, j, x);
        pl_px<K>(dv, j, d);
        acc[0] += fwd_px<K, SOFTMAX>(x, d, cw);
      }
    } else {
      pl_load<K>(lg, HW, x, p);
      pl_load<K>(dg, HW, d, p);
      acc[0] += fwd_px<K, SOFTMAX>(x, d, cw);
    }
  });
  pl_block_row<1>(acc, part);
}

// One 256-thread block: each sample's sum over its tiles (pl_sample_sum); the batch sum is taken in sample order.
// den = H W Kw.
__global__ __launch_bounds__(256) void bl_finalize_kernel(const float* part, int tiles, int N, double den,
                                                          float* loss, float* parts) {
  __shared__ double tot[64];
  const int tid = threadIdx.x;
  EUNET_DASSERT(N <= 64);
  for (int n = 0; n < N; ++n) {
    double v[1];
    pl_sample_sum<1>(part, tiles, n, v);
    if (tid == 0) {
      tot[n] = v[0];
      if (parts) parts[n] = (float)(v[0] / den);
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
      const Sig s = sigmoid_terms<false>(x[c]);
      g[c] = cw.w[c] * d[c] * (s.p * s.q);
    }
  }
}

// VEC: one thread per group of 4 pixels (HW % 4 == 0, so a group never straddles two samples).  inv = 1 / (N H W Kw)
template <int K, bool SOFTMAX, bool VEC>
__global__ __launch_bounds__(PL_NT) void bl_bwd_kernel(const float* logits, const float* dist, int N, int HW,
                                                       Weights cw, float inv, const float* gloss, float* glog) {
  constexpr int PER = VEC ? 4 : 1;
  long long id;
  int n, p;
  if (!pl_bwd_split<PER>(N, HW, id, n, p)) return;
  const long long at = (long long)n * K * HW + p;
  const float g0 = gloss[0] * inv;
  float x[K], d[K], g[K];
  if constexpr (VEC) {
    f32x4 xv[K], dv[K], gv[K];
    pl_load4<K>(logits + at, HW, xv);
    pl_load4<K>(dist + at, HW, dv);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      pl_px<K>(xv, j, x);
      pl_px<K>(dv, j, d);
      bwd_px<K, SOFTMAX>(x, d, cw, g);
#pragma unroll
      for (int c = 0; c < K; ++c) gv[c][j] = g0 * g[c];
    }
    pl_store4<K>(glog + at, HW, gv);
  } else {
    pl_load<K>(logits + at, HW, x);
    pl_load<K>(dist + at, HW, d);
    bwd_px<K, SOFTMAX>(x, d, cw, g);
#pragma unroll
    for (int c = 0; c < K; ++c) g[c] = g0 * g[c];
    pl_store<K>(glog + at, HW, g);
  }
}

// the shared argument rules of the two loss entries; fills cw and Kw
bool loss_args(const char* what, const void* a, const void* b, const void* c, const void* d, int n, int k, int h,
               int w, int activation, const float* class_weight, Weights* cw, int* kw) {
  if (!(a && b && c && d && pl_shape_ok(n, k, h, w))) {
    eunet::set_error("%s: bad args (" PL_SHAPE_RULE ")", what);
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

// f(K, SOFTMAX) for the (k, activation) that loss_args let through: no softmax kernel of K = 1 is built
template <class F>
void by_k_softmax(int k, int activation, F&& f) {
  by_k(k, [&](auto kc) {
    by_flag(activation == EUNET_BOUNDARY_SOFTMAX, [&](auto sc) {
      if constexpr (decltype(kc)::value > 1 || !decltype(sc)::value) f(kc, sc);
    });
  });
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
    remap_fg_kernel<<<grid_for(total, 2048), PL_NT, 0, s>>>(target, total, ign, fg);
    EUNET_LAUNCH_CHECK("signed_distance");
    sites = fg;
    values[0] = 1;
  }
  int rc = eunet_edt_sq(sites, n, h, w, values, k, EUNET_EDT_EQ, dout, stream);
  if (rc != EUNET_OK) return rc;
  rc = eunet_edt_sq(sites, n, h, w, values, k, EUNET_EDT_NE, din, stream);
  if (rc != EUNET_OK) return rc;
  const bool vec = pl_vec_ok(HW, {target, ws, out});
  const dim3 grid((unsigned)cdiv(HW, PL_NT * (vec ? 4 : 1)), (unsigned)n);
  const double cl = (double)clip, sc = (double)scale;
  by_k(k, [&](auto kc) {
    by_flag(vec, [&](auto vc) {
      sdf_combine_kernel<decltype(kc)::value, decltype(vc)::value>
          <<<grid, PL_NT, 0, s>>>(dout, din, target, HW, ign, cl, sc, out);
    });
  });
  return eunet::check_launch("signed_distance");
}

int eunet_boundary_loss_workspace_bytes(int n, int h, int w, size_t* bytes) {
  EUNET_REQUIRE(bytes && n > 0 && h > 0 && w > 0, "boundary_loss_workspace_bytes: bad args");
  *bytes = pl_workspace_bytes(n, h, w, 1);
  return EUNET_OK;
}

int eunet_boundary_loss_fwd(const float* logits, const float* dist, int n, int k, int h, int w, int activation,
                            const float* class_weight, float* loss, float* parts, void* ws, void* stream) {
  Weights cw;
  int kw;
  if (!loss_args("boundary_loss_fwd", logits, dist, loss, ws, n, k, h, w, activation, class_weight, &cw, &kw))
    return EUNET_ERR_INVALID;
  const int HW = h * w, tiles = pl_tiles(HW);
  const hipStream_t s = (hipStream_t)stream;
  float* part = (float*)ws;
  by_k_softmax(k, activation, [&](auto kc, auto sc) {
    by_flag(pl_vec_ok(HW, {logits, dist}), [&](auto vc) {
      bl_fwd_kernel<decltype(kc)::value, decltype(sc)::value, decltype(vc)::value>
          <<<dim3(tiles, n), PL_NT, 0, s>>>(logits, dist, HW, cw, part);
    });
  });
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
  const bool vec = pl_vec_ok(HW, {logits, dist, glogits});
  const hipStream_t s = (hipStream_t)stream;
  const float inv = (float)(1.0 / ((double)n * HW * kw));
  by_k_softmax(k, activation, [&](auto kc, auto sc) {
    by_flag(vec, [&](auto vc) {
      bl_bwd_kernel<decltype(kc)::value, decltype(sc)::value, decltype(vc)::value>
          <<<pl_bwd_grid(n, HW, vec), PL_NT, 0, s>>>(logits, dist, n, HW, cw, inv, gloss, glogits);
    });
  });
  return eunet::check_launch("boundary_loss_bwd");
}

}  // extern "C"
