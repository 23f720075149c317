// Combined segmentation loss, fused and batched (one launch for all samples).
//
// Reference: FocalLoss (train_eval.py:28-60; the Trainer builds it with alpha [1,8,5],
// gamma 5, CE class weights [1,20,10] at :74-79), Trainer.dice_loss (:134-157, weights
// [1,15,8]), Trainer.tversky_loss (:159-181, weights [1,12,6], alpha 0.7),
// _compute_combined_loss (:183-197; 2.5/2.5/1.0 at :82-85) and the per-sample loop + /B
// of Trainer.train_epoch (:262-337).
//   focal_n = mean_px alpha_t (1-pt)^gamma ce,  ce = -w_t log p_t,  pt = exp(-ce)
//   dice_n  = (1/D) sum_c wd_c (1 - (2 I_c + 1e-6)/(S_c + T_c + 1e-6))
//   tv_n    = (1/D) sum_c wt_c (1 - (I_c + 1e-6)/(I_c + a fp_c + (1-a) fn_c + 1e-6))
// with I = sum p t, S = sum p, T = sum t per (sample, class) and D the num_classes the
// reference divides by (3 in _compute_combined_loss for any K, :192-193; for K=2 this is
// exactly its K=3 loss with a third logit at -inf, pinned by tests/golden).
//   loss = w_focal * (sum_n sum_px focal) / F_den + (1/N) sum_n (w_dice dice_n + w_tv tv_n)
// F_den = N*H*W (the pixel mean of FocalLoss, and of the per-sample loop's mean over
// samples), or sum of w_t (nn.CrossEntropyLoss's weighted mean, focal_norm = 1).
// Pixels whose target is ignore_index contribute ce = 0 (F.cross_entropy ignore_index).
// Targets outside [0, K) that are not ignore_index are an error in the reference
// (F.cross_entropy raises / device-asserts): they are counted into sums[N*NV + 1] for the
// host to report at its next synchronisation, and contribute nothing here.
// Backward is analytic per pixel from the saved per-(sample,class) sums.
//
// WEIGHTED (eunet_loss_fwd_w / eunet_loss_bwd_w): the per-pixel focal summand is multiplied by a
// per-pixel weight m [N,H,W] (the U-Net border weight map of weightmap.hip), F_den stays N*H*W, Dice
// and Tversky are untouched.  The weight enters as a factor of alpha_t (forward) and of the finished
// focal coefficient (backward): a multiplication by 1.0f is exact and the rest of the expression is
// the unweighted one, so m = 1 gives the unweighted bits.  WEIGHTED = false is the code as it was.
#include "common.h"
#include "pixelloss.h"

EUNET_DEBUG_UNIT(loss)

namespace {
// the Trainer's enhanced_unet configuration (train_eval.py:74-87, 140, 164, 175)
const eunet_loss_params kReferenceParams = {
    {1.f, 20.f, 10.f}, {1.f, 8.f, 5.f}, 5.f, EUNET_NO_IGNORE, {1.f, 15.f, 8.f}, {1.f, 12.f, 6.f}, 0.7f, 2.5f, 2.5f, 1.f, 3.f, 0};

constexpr float EPS = 1e-6f;

// (1-pt)^gamma and (1-pt)^(gamma-1); gamma 5 (the reference's) in the product form the
// fixtures were pinned with, small integers by repeated products, otherwise powf
__device__ __forceinline__ void focal_pow(float om, float gamma, float& pg, float& pg1) {
  if (gamma == 5.f) {
    const float om2 = om * om, om4 = om2 * om2;
    pg = om4 * om;
    pg1 = om4;
    return;
  }
  const int gi = (int)gamma;
  if ((float)gi == gamma && gi >= 0 && gi <= 8) {
    float r = 1.f;
    for (int i = 1; i < gi; ++i) r *= om;
    pg1 = gi >= 1 ? r : 0.f;
    pg = gi >= 1 ? r * om : 1.f;
    return;
  }
  pg = powf(om, gamma);
  pg1 = powf(om, gamma - 1.f);
}

template <int K, bool WEIGHTED>
__global__ __launch_bounds__(PL_NT) void loss_fwd_kernel(const float* logits, const int64_t* target, const float* pw,
                                                         int HW, eunet_loss_params prm, float* part) {
  constexpr int NV = pl_nv(K);  // focal sum, I/S/T per class, ce-weight sum, bad-target count
  const int n = blockIdx.y;
  const long long plane = HW;
  const float* lg = logits + (long long)n * K * HW;
  const int64_t* tg = target + (long long)n * HW;
  float acc[NV];
#pragma unroll
  for (int i = 0; i < NV; ++i) acc[i] = 0.f;
  // the scalar visit of pl_tile_visit<false>, written out: through the callable the K = 3 kernel contracts three
  // more accumulations and its sums lose bit identity with the pinned ones (tools/bitcmp.py --losses)
  const int p0 = blockIdx.x * PL_LPIX;
  const int p1 = min(HW, p0 + PL_LPIX);
  for (int p = p0 + threadIdx.x; p < p1; p += PL_NT) {
    EUNET_DASSERT(p < HW);
    float x[K], pr[K], lse_m, m;
    pl_load<K>(lg, HW, x, p);
    softmax_px<K>(x, pr, m, lse_m);
    const int64_t traw = tg[p];
    const bool ign = traw == (int64_t)prm.ignore_index;
    const bool valid = !ign && traw >= 0 && traw < K;
    const int t = valid ? (int)traw : 0;
    if (valid) {
      const float logpt = lg[t * plane + p] - m - lse_m;
      const float ce = -prm.ce_weight[t] * logpt;
      const float pt = expf(-ce);
      float pg, pg1;
      focal_pow(1.f - pt, prm.gamma, pg, pg1);
      const float al = WEIGHTED ? pw[(long long)n * HW + p] * prm.alpha[t] : prm.alpha[t];
      acc[0] += al * pg * ce;
      acc[1 + 3 * K] += prm.ce_weight[t];
    } else if (!ign) {
      acc[2 + 3 * K] += 1.f;
    }
#pragma unroll
    for (int k = 0; k < K; ++k) {
      const float tk = (traw == (int64_t)k) ? 1.f : 0.f;
      acc[1 + k] += pr[k] * tk;
      acc[1 + K + k] += pr[k];
      acc[1 + 2 * K + k] += tk;
    }
  }
  pl_block_row<NV>(acc, part);
}

// One 256-thread block: thread 0 forms each sample's terms from its sums (pl_sample_sum); the batch sums are
// taken in sample order.
template <int K>
__global__ __launch_bounds__(256) void loss_finalize_kernel(const float* part, int tiles, int N, int HW,
                                                            eunet_loss_params prm, float* sums, float* loss,
                                                            float* parts) {
  constexpr int NV = pl_nv(K);
  __shared__ double per[64], fnum[64], fden[64], nbad[64];
  const int tid = threadIdx.x;
  EUNET_DASSERT(N <= 64);
  for (int n = 0; n < N; ++n) {
    double v[NV];
    pl_sample_sum<NV>(part, tiles, n, v);
    if (tid == 0) {
#pragma unroll
      for (int i = 0; i < NV; ++i) sums[n * NV + i] = (float)v[i];
      double dice = 0.0, tv = 0.0;
      for (int k = 0; k < K; ++k) {
        const double I = v[1 + k], S = v[1 + K + k], T = v[1 + 2 * K + k];
        dice += prm.dice_weight[k] * (1.0 - (2.0 * I + EPS) / (S + T + EPS));
        const double fp = S - I, fn = T - I;
        const double a = prm.tversky_alpha;
        tv += prm.tversky_weight[k] * (1.0 - (I + EPS) / (I + a * fp + (1.0 - a) * fn + EPS));
      }
      dice /= prm.class_div;
      tv /= prm.class_div;
      const double den = prm.focal_norm ? v[1 + 3 * K] : (double)HW;
      if (parts) {
        parts[n * 3 + 0] = (float)(v[0] / den);
        parts[n * 3 + 1] = (float)dice;
        parts[n * 3 + 2] = (float)tv;
      }
      per[n] = prm.w_dice * dice + prm.w_tversky * tv;
      fnum[n] = v[0];
      fden[n] = den;
      nbad[n] = v[2 + 3 * K];
    }
    __syncthreads();
  }
  if (tid == 0) {
    double s = 0.0, fn = 0.0, fd = 0.0, nb = 0.0;
    for (int i = 0; i < N; ++i) {
      s += per[i];
      fn += fnum[i];
      fd += fden[i];
      nb += nbad[i];
    }
    const double focal = fd > 0.0 ? fn / fd : 0.0;  // all pixels ignored: F.cross_entropy's mean is nan; 0 here
    loss[0] = (float)(prm.w_focal * focal + s / (double)N);
    sums[N * NV] = (float)fd;
    sums[N * NV + 1] = (float)nb;
  }
}

template <int K, bool WEIGHTED>
__global__ void loss_bwd_kernel(const float* logits, const int64_t* target, const float* pw, int N, int HW,
                                eunet_loss_params prm, const float* sums, const float* gloss, float* glog) {
  constexpr int NV = pl_nv(K);
  long long id;
  int n, p;
  if (!pl_bwd_split<1>(N, HW, id, n, p)) return;
  const long long plane = HW;
  const float* lg = logits + (long long)n * K * HW + p;
  float x[K], pr[K], lse_m, m;
  pl_load<K>(lg, HW, x);
  softmax_px<K>(x, pr, m, lse_m);
  const int64_t traw = target[id];
  const bool valid = traw != (int64_t)prm.ignore_index && traw >= 0 && traw < K;
  const int t = valid ? (int)traw : 0;
  float fcoef = 0.f;  // d (w_focal * focal term) / d ce * w_t
  if (valid) {
    const float logpt = lg[t * plane] - m - lse_m;
    const float ce = -prm.ce_weight[t] * logpt;
    const float pt = expf(-ce);
    float pg, pg1;
    focal_pow(1.f - pt, prm.gamma, pg, pg1);
    const float dfdce = prm.alpha[t] * (pg + ce * prm.gamma * pg1 * pt);
    fcoef = prm.w_focal * dfdce * prm.ce_weight[t] / sums[N * NV];
    if (WEIGHTED) fcoef *= pw[id];
  }
  const float invn = 1.f / (float)N;
  const float* sm = sums + n * NV;
  float dp[K];
  float sdp = 0.f;
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const float I = sm[1 + k], S = sm[1 + K + k], T = sm[1 + 2 * K + k];
    const float tk = (traw == (int64_t)k) ? 1.f : 0.f;
    const float ud = S + T + EPS;
    const float dd = (prm.dice_weight[k] / prm.class_div) * (-2.f * tk / ud + (2.f * I + EPS) / (ud * ud));
    const float a = prm.tversky_alpha;
    const float den = I + a * (S - I) + (1.f - a) * (T - I) + EPS;
    const float dt = -(prm.tversky_weight[k] / prm.class_div) * (tk / den - a * (I + EPS) / (den * den));
    dp[k] = prm.w_dice * dd + prm.w_tversky * dt;
    sdp += pr[k] * dp[k];
  }
  const float g0 = gloss[0];
  // stored from the loop, not staged for pl_store: staged, the K = 3 kernel contracts the other product of g
  // into its multiply-add and a last bit changes (tools/bitcmp.py --losses)
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const float tk = (valid && t == k) ? 1.f : 0.f;
    const float g = invn * pr[k] * (dp[k] - sdp) + fcoef * (pr[k] - tk);
    glog[(long long)n * K * HW + k * plane + p] = g * g0;
  }
}

}  // namespace

extern "C" {

int eunet_loss_reference_params(eunet_loss_params* prm) {
  EUNET_REQUIRE(prm, "loss_reference_params: null");
  *prm = kReferenceParams;
  return EUNET_OK;
}

int eunet_loss_sums_len(int n, int k, int* len) {
  EUNET_REQUIRE(len && n > 0 && k >= 1 && k <= 3, "loss_sums_len: bad args");
  *len = pl_sums_len(n, pl_nv(k));
  return EUNET_OK;
}

int eunet_loss_workspace_bytes(int n, int k, int h, int w, size_t* bytes) {
  EUNET_REQUIRE(bytes && n > 0 && k >= 1 && k <= 3 && h > 0 && w > 0, "loss_workspace_bytes: bad args");
  *bytes = pl_workspace_bytes(n, h, w, pl_nv(k));
  return EUNET_OK;
}

}  // extern "C"

// one launcher per direction for the unweighted and the weighted entry points (pw == nullptr: unweighted)
namespace {
int loss_fwd_launch(const float* logits, const int64_t* target, const float* pw, int n, int k, int h, int w,
                    const eunet_loss_params* params, float* sums, float* loss, float* parts, void* ws, void* stream,
                    const char* what) {
  EUNET_REQUIRE(logits && target && sums && loss && ws && pl_shape_ok(n, k, h, w), "%s: bad args (" PL_SHAPE_RULE ")",
                what);
  const eunet_loss_params prm = params ? *params : kReferenceParams;
  EUNET_REQUIRE(prm.class_div > 0.f, "%s: class_div must be > 0", what);
  EUNET_REQUIRE(!pw || prm.focal_norm == 0,
                "%s: focal_norm = 1 with a pixel weight is not defined (its denominator would need a definition)", what);
  const int HW = h * w, tiles = pl_tiles(HW);
  hipStream_t s = (hipStream_t)stream;
  by_k(k, [&](auto kc) {
    constexpr int K = decltype(kc)::value;
    by_flag(pw != nullptr, [&](auto wc) {
      loss_fwd_kernel<K, decltype(wc)::value><<<dim3(tiles, n), PL_NT, 0, s>>>(logits, target, pw, HW, prm, (float*)ws);
    });
    loss_finalize_kernel<K><<<1, 256, 0, s>>>((const float*)ws, tiles, n, HW, prm, sums, loss, parts);
  });
  return eunet::check_launch(what);
}

int loss_bwd_launch(const float* logits, const int64_t* target, const float* pw, int n, int k, int h, int w,
                    const eunet_loss_params* params, const float* sums, const float* gloss, float* glogits,
                    void* stream, const char* what) {
  EUNET_REQUIRE(logits && target && sums && gloss && glogits && pl_shape_ok(n, k, h, w),
                "%s: bad args (" PL_SHAPE_RULE ")", what);
  const eunet_loss_params prm = params ? *params : kReferenceParams;
  EUNET_REQUIRE(!pw || prm.focal_norm == 0, "%s: focal_norm = 1 with a pixel weight is not defined", what);
  hipStream_t s = (hipStream_t)stream;
  by_k(k, [&](auto kc) {
    by_flag(pw != nullptr, [&](auto wc) {
      loss_bwd_kernel<decltype(kc)::value, decltype(wc)::value><<<pl_bwd_grid(n, h * w, false), PL_NT, 0, s>>>(
          logits, target, pw, n, h * w, prm, sums, gloss, glogits);
    });
  });
  return eunet::check_launch(what);
}
}  // namespace

extern "C" {

int eunet_loss_fwd(const float* logits, const int64_t* target, int n, int k, int h, int w,
                   const eunet_loss_params* params, float* sums, float* loss, float* parts, void* ws, void* stream) {
  return loss_fwd_launch(logits, target, nullptr, n, k, h, w, params, sums, loss, parts, ws, stream, "loss_fwd");
}

int eunet_loss_fwd_w(const float* logits, const int64_t* target, const float* pixel_weight, int n, int k, int h, int w,
                     const eunet_loss_params* params, float* sums, float* loss, float* parts, void* ws,
                     void* stream) {
  EUNET_REQUIRE(pixel_weight, "loss_fwd_w: pixel_weight must not be null");
  return loss_fwd_launch(logits, target, pixel_weight, n, k, h, w, params, sums, loss, parts, ws, stream,
                         "loss_fwd_w");
}

int eunet_loss_bwd(const float* logits, const int64_t* target, int n, int k, int h, int w,
                   const eunet_loss_params* params, const float* sums, const float* gloss, float* glogits,
                   void* stream) {
  return loss_bwd_launch(logits, target, nullptr, n, k, h, w, params, sums, gloss, glogits, stream, "loss_bwd");
}

int eunet_loss_bwd_w(const float* logits, const int64_t* target, const float* pixel_weight, int n, int k, int h, int w,
                     const eunet_loss_params* params, const float* sums, const float* gloss, float* glogits,
                     void* stream) {
  EUNET_REQUIRE(pixel_weight, "loss_bwd_w: pixel_weight must not be null");
  return loss_bwd_launch(logits, target, pixel_weight, n, k, h, w, params, sums, gloss, glogits, stream,
                         "loss_bwd_w");
}

}  // extern "C"
