// Sigmoid BCE + soft Dice loss for binary and multi-label training, fused and batched, and the
// sigmoid prediction path of the evaluator.
//
// No reference line to cite: the reference has no BCE.  The source is the
// project's own statement of purpose, BASELINE.json north_star ("BCE/Dice" per-pixel loss); the
// definition is the one in include/eunet.h (eunet_bce_dice_fwd):
//   sp(z)  = max(z, 0) + log1p(exp(-|z|)),  sig = sigmoid
//   bce_c  = cw_c (pw_c t_c sp(-x_c) + (1 - t_c) sp(x_c))     (F.binary_cross_entropy_with_logits)
//   BCE    = sum_{n,c,valid px} bce / (K max(1, V)),  V = number of valid pixels of the batch
//   dice_n = (1/K) sum_c dw_c (1 - (2 I + s)/(S + T + s)),  I = sum sig t, S = sum sig, T = sum t
//   loss   = w_bce BCE + w_dice (1/N) sum_n dice_n
// t_c = [target == c] (onehot) or t_0 = [target >= 1] (foreground, K = 1).  A pixel at ignore_index
// contributes to nothing -- not to the BCE sum, its denominator, I, S or T.  (loss.hip differs: there
// an ignored pixel's probability still counts in S.)  A pixel that is neither valid nor ignored
// contributes nothing either and is counted into the last element of sums, where eunet_loss_fwd
// puts its count.
//
// Three HBM-bound streams.  Forward: one block per (sample, tile of 1024 pixels) reads the logits and
// the target once (16 bytes per lane when H*W is a multiple of 4), reduces in the wave and writes one
// partial row; a single block sums the partials in fp64 in a fixed order (deterministic).  Backward:
// analytic per pixel from the saved sums, logits and target read once, the gradient written once.
//
// WEIGHTED (eunet_bce_dice_fwd_w / _bwd_w): bce(x,t)_c is multiplied by a per-pixel weight m [N,H,W] (one
// more stream, read 16 bytes per lane on the vector path); the denominators and the Dice terms are
// untouched.  The weight enters as a factor of cw_c (forward) and of the BCE coefficient (backward): a
// multiplication by 1.0f is exact and the rest of the expression is the unweighted one, so m = 1 gives the
// unweighted bits.  WEIGHTED = false is the code as it was.
#include "common.h"
#include "pixelloss.h"
#include "labelmap.h"

EUNET_DEBUG_UNIT(bcedice)

namespace {
typedef long long i64x2 __attribute__((ext_vector_type(2)));

const eunet_bce_dice_params kDefaultParams = {
    {1.f, 1.f, 1.f}, {1.f, 1.f, 1.f}, {1.f, 1.f, 1.f}, 1.f, 1.f, 1e-6f, EUNET_NO_IGNORE, EUNET_BCE_TARGET_AUTO};

// 0 ignored, 1 valid, 2 out of range
__device__ __forceinline__ int classify(int64_t traw, int K, const eunet_bce_dice_params& prm) {
  if (traw == (int64_t)prm.ignore_index) return 0;
  const bool ok = prm.target_mode == EUNET_BCE_TARGET_FOREGROUND ? traw >= 0 : (traw >= 0 && traw < K);
  return ok ? 1 : 2;
}

__device__ __forceinline__ float target_of(int64_t traw, int c, const eunet_bce_dice_params& prm) {
  const bool on = prm.target_mode == EUNET_BCE_TARGET_FOREGROUND ? traw >= 1 : traw == (int64_t)c;
  return on ? 1.f : 0.f;
}

// acc: [0] bce sum, [1+c] I, [1+K+c] S, [1+2K+c] T, [1+3K] valid pixels, [2+3K] out-of-range targets
template <int K, bool WEIGHTED>
__device__ __forceinline__ void fwd_px(const float (&x)[K], int64_t traw, float wt, const eunet_bce_dice_params& prm,
                                       float (&acc)[3 + 3 * K]) {
  const int cls = classify(traw, K, prm);
  if (cls == 2) acc[2 + 3 * K] += 1.f;
  if (cls != 1) return;
  acc[1 + 3 * K] += 1.f;
#pragma unroll
  for (int c = 0; c < K; ++c) {
    const Sig s = sigmoid_terms<true>(x[c]);
    const float t = target_of(traw, c, prm);
    const float cw = WEIGHTED ? wt * prm.class_weight[c] : prm.class_weight[c];
    acc[0] += cw * (prm.pos_weight[c] * t * s.spn + (1.f - t) * s.spp);
    acc[1 + c] += s.p * t;
    acc[1 + K + c] += s.p;
    acc[1 + 2 * K + c] += t;
  }
}

// The visit and the loads are written out here, not taken from pixelloss.h (pl_tile_visit, pl_load4, pl_px): through
// them the compiler packs and contracts the accumulations differently and K = 3 takes one more register, across a
// waves-per-SIMD step (profiles/pixelloss_resources.txt).  The tail is the shared one.
template <int K, bool VEC, bool WEIGHTED>
__global__ __launch_bounds__(PL_NT) void bce_dice_fwd_kernel(const float* logits, const int64_t* target,
                                                             const float* pw, int HW, eunet_bce_dice_params prm,
                                                             float* part) {
  constexpr int NV = pl_nv(K);
  const int n = blockIdx.y, tid = threadIdx.x;
  const float* lg = logits + (long long)n * K * HW;
  const int64_t* tg = target + (long long)n * HW;
  const float* wg = WEIGHTED ? pw + (long long)n * HW : nullptr;
  float acc[NV];
#pragma unroll
  for (int i = 0; i < NV; ++i) acc[i] = 0.f;
  const int p0 = blockIdx.x * PL_LPIX;
  const int p1 = min(HW, p0 + PL_LPIX);
  if (VEC) {  // HW % 4 == 0: every plane and every 4-pixel group starts on 16 bytes
    const int p = p0 + tid * 4;
    if (p < p1) {
      EUNET_DASSERT(p + 3 < HW);
      f32x4 xv[K];
#pragma unroll
      for (int c = 0; c < K; ++c) xv[c] = *reinterpret_cast<const f32x4*>(lg + (long long)c * HW + p);
      const i64x2 t01 = *reinterpret_cast<const i64x2*>(tg + p);
      const i64x2 t23 = *reinterpret_cast<const i64x2*>(tg + p + 2);
      const int64_t tr[4] = {t01[0], t01[1], t23[0], t23[1]};
      f32x4 wv = {1.f, 1.f, 1.f, 1.f};
      if (WEIGHTED) wv = *reinterpret_cast<const f32x4*>(wg + p);
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        float x[K];
#pragma unroll
        for (int c = 0; c < K; ++c) x[c] = xv[c][j];
        fwd_px<K, WEIGHTED>(x, tr[j], wv[j], prm, acc);
      }
    }
  } else {
    for (int p = p0 + tid; p < p1; p += PL_NT) {
      EUNET_DASSERT(p < HW);
      float x[K];
#pragma unroll
      for (int c = 0; c < K; ++c) x[c] = lg[(long long)c * HW + p];
      fwd_px<K, WEIGHTED>(x, tg[p], WEIGHTED ? wg[p] : 1.f, prm, acc);
    }
  }
  pl_block_row<NV>(acc, part);
}

// One 256-thread block: thread 0 forms each sample's terms from its sums (pl_sample_sum); the batch sums are
// taken in sample order.
template <int K>
__global__ __launch_bounds__(256) void bce_dice_finalize_kernel(const float* part, int tiles, int N,
                                                                eunet_bce_dice_params prm, float* sums,
                                                                float* loss, float* parts) {
  constexpr int NV = pl_nv(K);
  __shared__ double dice_s[64], bnum[64], vcnt[64], nbad[64];
  const int tid = threadIdx.x;
  EUNET_DASSERT(N <= 64);
  for (int n = 0; n < N; ++n) {
    double v[NV];
    pl_sample_sum<NV>(part, tiles, n, v);
    if (tid == 0) {
#pragma unroll
      for (int i = 0; i < NV; ++i) sums[n * NV + i] = (float)v[i];
      const double sm = (double)prm.smooth;
      double dice = 0.0;
      for (int c = 0; c < K; ++c) {
        const double I = v[1 + c], S = v[1 + K + c], T = v[1 + 2 * K + c];
        dice += prm.dice_weight[c] * (1.0 - (2.0 * I + sm) / (S + T + sm));
      }
      dice /= (double)K;
      const double vn = v[1 + 3 * K];
      if (parts) {
        parts[n * 2 + 0] = (float)(v[0] / ((double)K * (vn > 1.0 ? vn : 1.0)));
        parts[n * 2 + 1] = (float)dice;
      }
      dice_s[n] = dice;
      bnum[n] = v[0];
      vcnt[n] = vn;
      nbad[n] = v[2 + 3 * K];
    }
    __syncthreads();
  }
  if (tid == 0) {
    double d = 0.0, b = 0.0, vt = 0.0, nb = 0.0;
    for (int i = 0; i < N; ++i) {
      d += dice_s[i];
      b += bnum[i];
      vt += vcnt[i];
      nb += nbad[i];
    }
    const double bce = b / ((double)K * (vt > 1.0 ? vt : 1.0));  // no valid pixel: b = 0, the loss is 0
    loss[0] = (float)(prm.w_bce * bce + prm.w_dice * d / (double)N);
    sums[N * NV] = (float)vt;
    sums[N * NV + 1] = (float)nb;
  }
}

// per (sample, class): the Dice gradient is (a t + b) sig(x) sig(-x)
template <int K>
struct DiceCoef {
  float a[K], b[K];
};
template <int K>
__device__ __forceinline__ DiceCoef<K> dice_coef(const float* sm, int N, const eunet_bce_dice_params& prm) {
  DiceCoef<K> d;
#pragma unroll
  for (int c = 0; c < K; ++c) {
    const float I = sm[1 + c], S = sm[1 + K + c], T = sm[1 + 2 * K + c];
    const float u = S + T + prm.smooth;
    const float w = prm.w_dice * prm.dice_weight[c] / (float)(N * K);
    d.a[c] = -2.f * w / u;
    d.b[c] = w * (2.f * I + prm.smooth) / (u * u);
  }
  return d;
}

template <int K>
__device__ __forceinline__ void bwd_px(const float (&x)[K], int64_t traw, const eunet_bce_dice_params& prm,
                                       const DiceCoef<K>& dc, float cb, float g0, float (&g)[K]) {
  const bool valid = classify(traw, K, prm) == 1;
#pragma unroll
  for (int c = 0; c < K; ++c) {
    const Sig s = sigmoid_terms<false>(x[c]);
    const float t = target_of(traw, c, prm);
    const float gb = cb * prm.class_weight[c] * (-prm.pos_weight[c] * t * s.q + (1.f - t) * s.p);
    const float gd = (dc.a[c] * t + dc.b[c]) * s.p * s.q;
    g[c] = valid ? g0 * (gb + gd) : 0.f;
  }
}

// VEC: one thread per group of 4 pixels (HW % 4 == 0, so a group never straddles two samples)
// WEIGHTED: bwd_px gets cb * m(x) for cb
template <int K, bool VEC, bool WEIGHTED>
__global__ __launch_bounds__(PL_NT) void bce_dice_bwd_kernel(const float* logits, const int64_t* target,
                                                             const float* pw, int N, int HW,
                                                             eunet_bce_dice_params prm, const float* sums,
                                                             const float* gloss, float* glog) {
  constexpr int NV = pl_nv(K), PER = VEC ? 4 : 1;
  long long id;
  int n, p;
  if (!pl_bwd_split<PER>(N, HW, id, n, p)) return;
  const DiceCoef<K> dc = dice_coef<K>(sums + n * NV, N, prm);
  const float vt = sums[N * NV];
  const float cb = prm.w_bce / ((float)K * fmaxf(vt, 1.f));
  const float g0 = gloss[0];
  const float* lg = logits + (long long)n * K * HW + p;
  float* gl = glog + (long long)n * K * HW + p;
  if (VEC) {
    f32x4 xv[K], gv[K], wv[1] = {{1.f, 1.f, 1.f, 1.f}};
    int64_t tr[4];
    pl_load4<K>(lg, HW, xv);
    pl_load4(target + id, tr);
    if (WEIGHTED) pl_load4<1>(pw + id, HW, wv);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      float x[K], g[K];
      pl_px<K>(xv, j, x);
      bwd_px<K>(x, tr[j], prm, dc, WEIGHTED ? cb * wv[0][j] : cb, g0, g);
#pragma unroll
      for (int c = 0; c < K; ++c) gv[c][j] = g[c];
    }
    pl_store4<K>(gl, HW, gv);
  } else {
    float x[K], g[K];
    pl_load<K>(lg, HW, x);
    bwd_px<K>(x, target[id], prm, dc, WEIGHTED ? cb * pw[id] : cb, g0, g);
    pl_store<K>(gl, HW, g);
  }
}

template <int K>
__global__ __launch_bounds__(PL_NT) void sigmoid_crop_kernel(const float* logits, int hp, int wp, int h, int w,
                                                          int flip_h, int flip_w, float* probs) {
  const long long total = (long long)h * w;
  for (long long id = (long long)blockIdx.x * PL_NT + threadIdx.x; id < total; id += (long long)gridDim.x * PL_NT) {
    const int x = (int)(id % w), yy = (int)(id / w);
    const int sy = flip_h ? h - 1 - yy : yy, sx = flip_w ? w - 1 - x : x;
    EUNET_DASSERT(sy >= 0 && sy < hp && sx >= 0 && sx < wp);
    const long long s = (long long)sy * wp + sx;
#pragma unroll
    for (int k = 0; k < K; ++k) probs[(long long)k * total + id] = sigmoid_terms<false>(logits[(long long)k * hp * wp + s]).p;
  }
}

template <int K>
__global__ __launch_bounds__(PL_NT) void probs_threshold_kernel(const float* probs, long long hw, float thr,
                                                                int64_t* mask) {
  for (long long id = (long long)blockIdx.x * PL_NT + threadIdx.x; id < hw; id += (long long)gridDim.x * PL_NT) {
    int64_t m;
    if (K == 1) {
      m = probs[id] >= thr ? 1 : 0;
    } else {
      float best = probs[id];
      m = 0;
#pragma unroll
      for (int k = 1; k < K; ++k) {
        const float v = probs[(long long)k * hw + id];
        if (v > best) {  // strict: the first maximum wins a tie
          best = v;
          m = k;
        }
      }
    }
    mask[id] = m;
  }
}

// the params of a call with target_mode resolved for K; false (error set) when they are refused
bool resolve(const eunet_bce_dice_params* params, int k, eunet_bce_dice_params* out, const char* what) {
  *out = params ? *params : kDefaultParams;
  if (out->target_mode == EUNET_BCE_TARGET_AUTO)
    out->target_mode = k == 1 ? EUNET_BCE_TARGET_FOREGROUND : EUNET_BCE_TARGET_ONEHOT;
  if (out->target_mode == EUNET_BCE_TARGET_FOREGROUND ? k != 1 : (out->target_mode != EUNET_BCE_TARGET_ONEHOT || k == 1)) {
    eunet::set_error("%s: target_mode %d with K = %d (foreground is the mode of K = 1, and its only one)", what,
                     out->target_mode, k);
    return false;
  }
  if (!(out->smooth > 0.f)) {
    eunet::set_error("%s: smooth must be > 0", what);
    return false;
  }
  return true;
}

// one launcher per direction for the unweighted and the weighted entry points (pw == nullptr: unweighted)
int bce_dice_fwd_launch(const float* logits, const int64_t* target, const float* pw, int n, int k, int h, int w,
                        const eunet_bce_dice_params* params, float* sums, float* loss, float* parts, void* ws,
                        void* stream, const char* what) {
  EUNET_REQUIRE(logits && target && sums && loss && ws && pl_shape_ok(n, k, h, w), "%s: bad args (" PL_SHAPE_RULE ")",
                what);
  eunet_bce_dice_params prm;
  if (!resolve(params, k, &prm, what)) return EUNET_ERR_INVALID;
  const int HW = h * w, tiles = pl_tiles(HW);
  hipStream_t s = (hipStream_t)stream;
  by_k(k, [&](auto kc) {
    constexpr int K = decltype(kc)::value;
    by_flag(pl_vec_ok(HW, {logits, target, pw}), [&](auto vc) {
      by_flag(pw != nullptr, [&](auto wc) {
        bce_dice_fwd_kernel<K, decltype(vc)::value, decltype(wc)::value>
            <<<dim3(tiles, n), PL_NT, 0, s>>>(logits, target, pw, HW, prm, (float*)ws);
      });
    });
    bce_dice_finalize_kernel<K><<<1, 256, 0, s>>>((const float*)ws, tiles, n, prm, sums, loss, parts);
  });
  return eunet::check_launch(what);
}

int bce_dice_bwd_launch(const float* logits, const int64_t* target, const float* pw, int n, int k, int h, int w,
                        const eunet_bce_dice_params* params, const float* sums, const float* gloss, float* glogits,
                        void* stream, const char* what) {
  EUNET_REQUIRE(logits && target && sums && gloss && glogits && pl_shape_ok(n, k, h, w),
                "%s: bad args (" PL_SHAPE_RULE ")", what);
  eunet_bce_dice_params prm;
  if (!resolve(params, k, &prm, what)) return EUNET_ERR_INVALID;
  const int HW = h * w;
  const bool vec = pl_vec_ok(HW, {logits, target, glogits, pw});
  hipStream_t s = (hipStream_t)stream;
  by_k(k, [&](auto kc) {
    by_flag(vec, [&](auto vc) {
      by_flag(pw != nullptr, [&](auto wc) {
        bce_dice_bwd_kernel<decltype(kc)::value, decltype(vc)::value, decltype(wc)::value>
            <<<pl_bwd_grid(n, HW, vec), PL_NT, 0, s>>>(logits, target, pw, n, HW, prm, sums, gloss, glogits);
      });
    });
  });
  return eunet::check_launch(what);
}

}  // namespace

extern "C" {

int eunet_bce_dice_default_params(eunet_bce_dice_params* prm) {
  EUNET_REQUIRE(prm, "bce_dice_default_params: null");
  *prm = kDefaultParams;
  return EUNET_OK;
}

int eunet_bce_dice_sums_len(int n, int k, int* len) {
  EUNET_REQUIRE(len && n > 0 && k >= 1 && k <= 3, "bce_dice_sums_len: bad args");
  *len = pl_sums_len(n, pl_nv(k));
  return EUNET_OK;
}

int eunet_bce_dice_workspace_bytes(int n, int k, int h, int w, size_t* bytes) {
  EUNET_REQUIRE(bytes && n > 0 && k >= 1 && k <= 3 && h > 0 && w > 0, "bce_dice_workspace_bytes: bad args");
  *bytes = pl_workspace_bytes(n, h, w, pl_nv(k));
  return EUNET_OK;
}

int eunet_bce_dice_fwd(const float* logits, const int64_t* target, int n, int k, int h, int w,
                       const eunet_bce_dice_params* params, float* sums, float* loss, float* parts, void* ws,
                       void* stream) {
  return bce_dice_fwd_launch(logits, target, nullptr, n, k, h, w, params, sums, loss, parts, ws, stream,
                             "bce_dice_fwd");
}

int eunet_bce_dice_fwd_w(const float* logits, const int64_t* target, const float* pixel_weight, int n, int k, int h,
                         int w, const eunet_bce_dice_params* params, float* sums, float* loss, float* parts, void* ws,
                         void* stream) {
  EUNET_REQUIRE(pixel_weight, "bce_dice_fwd_w: pixel_weight must not be null");
  return bce_dice_fwd_launch(logits, target, pixel_weight, n, k, h, w, params, sums, loss, parts, ws, stream,
                             "bce_dice_fwd_w");
}

int eunet_bce_dice_bwd(const float* logits, const int64_t* target, int n, int k, int h, int w,
                       const eunet_bce_dice_params* params, const float* sums, const float* gloss, float* glogits,
                       void* stream) {
  return bce_dice_bwd_launch(logits, target, nullptr, n, k, h, w, params, sums, gloss, glogits, stream,
                             "bce_dice_bwd");
}

int eunet_bce_dice_bwd_w(const float* logits, const int64_t* target, const float* pixel_weight, int n, int k, int h,
                         int w, const eunet_bce_dice_params* params, const float* sums, const float* gloss,
                         float* glogits, void* stream) {
  EUNET_REQUIRE(pixel_weight, "bce_dice_bwd_w: pixel_weight must not be null");
  return bce_dice_bwd_launch(logits, target, pixel_weight, n, k, h, w, params, sums, gloss, glogits, stream,
                             "bce_dice_bwd_w");
}

int eunet_sigmoid_crop(const float* logits, int k, int hp, int wp, int h, int w, int flip_h, int flip_w,
                       float* probs, void* stream) {
  EUNET_REQUIRE(logits && probs && k >= 1 && k <= 3 && h > 0 && w > 0 && h <= hp && w <= wp,
                "sigmoid_crop: bad args (K must be 1..3, crop inside the map)");
  hipStream_t s = (hipStream_t)stream;
  by_k(k, [&](auto kc) {
    sigmoid_crop_kernel<decltype(kc)::value>
        <<<grid_for((long long)h * w, 2048), PL_NT, 0, s>>>(logits, hp, wp, h, w, flip_h, flip_w, probs);
  });
  return eunet::check_launch("sigmoid_crop");
}

int eunet_probs_threshold(const float* probs, int k, int h, int w, float threshold, int64_t* mask, void* stream) {
  EUNET_REQUIRE(probs && mask && k >= 1 && k <= 3 && h > 0 && w > 0, "probs_threshold: bad args (K must be 1..3)");
  const long long hw = (long long)h * w;
  hipStream_t s = (hipStream_t)stream;
  by_k(k, [&](auto kc) {
    probs_threshold_kernel<decltype(kc)::value><<<grid_for(hw, 2048), PL_NT, 0, s>>>(probs, hw, threshold, mask);
  });
  return eunet::check_launch("probs_threshold");
}

}  // extern "C"
