// Kernels of the unet baseline that the Enhanced-UNet path does not have: the K-channel fp32 tails behind the
// 1x1 head (HBM-bound streams) -- the x2 upsample of dec1's output (models.py:236, dec1 commuted before it), the
// training loop's 2H -> H resize of it (train_eval.py:306-310), and their adjoints.
#include "common.h"

EUNET_DEBUG_UNIT(baselines)

namespace {

// ---------------------------------------------------------------------------
// K-channel fp32 tails.  z_lo [N,h,w,K] NHWC; outputs NCHW.
// ---------------------------------------------------------------------------
// the three taps of the 2H -> H resize of an x2 upsample along one axis: mean of the high-res positions 2i, 2i+1 =
// (1/8, 3/4, 1/8) over low-res i-1, i, i+1 with replicate edges (the clamped taps fold into the centre weight)
struct Tap3 { int i[3]; float w[3]; };
__device__ __forceinline__ Tap3 smooth_taps(int i, int n) {
  Tap3 t;
  t.i[0] = max(i - 1, 0); t.i[1] = i; t.i[2] = min(i + 1, n - 1);
  t.w[0] = 0.125f; t.w[1] = 0.75f; t.w[2] = 0.125f;
  return t;
}
// its transpose: the weights of g[i-1], g[i], g[i+1] in gz[i]; an edge keeps the eighth its clamped tap sent back
// to it (centre 7/8, 1 at n = 1) and has no neighbour beyond it
__device__ __forceinline__ Tap3 smooth_adj_taps(int i, int n) {
  Tap3 t;
  t.i[0] = max(i - 1, 0); t.i[1] = i; t.i[2] = min(i + 1, n - 1);
  t.w[0] = i > 0 ? 0.125f : 0.f;
  t.w[2] = i < n - 1 ? 0.125f : 0.f;
  t.w[1] = 0.75f + (i == 0 ? 0.125f : 0.f) + (i == n - 1 ? 0.125f : 0.f);
  return t;
}

// UP2: out [N,K,2h,2w] = up2(z_lo); one thread per high-res pixel, lanes along x (the NCHW stores of each class
// are coalesced; the K-float pixel loads of neighbouring lanes share their lines)
template <int K>
__global__ __launch_bounds__(256) void ktail_up2_fwd_kernel(const float* zlo, int N, int h, int w, float* out) {
  const int H2 = 2 * h, W2 = 2 * w;
  const long long id = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (id >= (long long)N * H2 * W2) return;
  const int X = (int)(id % W2);
  const int Y = (int)((id / W2) % H2);
  const int n = (int)(id / ((long long)W2 * H2));
  int y0, y1, x0, x1;
  float ly, lx;
  up2_src_i(Y, h, y0, y1, ly);
  up2_src_i(X, w, x0, x1, lx);
  EUNET_DASSERT(y0 >= 0 && y1 < h && x0 >= 0 && x1 < w);
  const float* r0 = zlo + ((long long)n * h + y0) * w * K;
  const float* r1 = zlo + ((long long)n * h + y1) * w * K;
  const float w00 = (1.f - ly) * (1.f - lx), w01 = (1.f - ly) * lx, w10 = ly * (1.f - lx), w11 = ly * lx;
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const float v = w00 * r0[x0 * K + k] + w01 * r0[x1 * K + k] + w10 * r1[x0 * K + k] + w11 * r1[x1 * K + k];
    __builtin_nontemporal_store(v, out + (((long long)n * K + k) * H2 + Y) * W2 + X);
  }
}

// SMOOTH: out [N,K,h,w] = mean2x2(up2(z_lo)) as the separable replicate-edge (1/8, 3/4, 1/8) filter
template <int K>
__global__ __launch_bounds__(256) void ktail_smooth_fwd_kernel(const float* zlo, int N, int h, int w, float* out) {
  const long long id = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (id >= (long long)N * h * w) return;
  const int x = (int)(id % w);
  const int y = (int)((id / w) % h);
  const int n = (int)(id / ((long long)w * h));
  const Tap3 ty = smooth_taps(y, h), tx = smooth_taps(x, w);
  float acc[K];
#pragma unroll
  for (int k = 0; k < K; ++k) acc[k] = 0.f;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const float* row = zlo + ((long long)n * h + ty.i[a]) * w * K;
#pragma unroll
    for (int b = 0; b < 3; ++b) {
      const float ww = ty.w[a] * tx.w[b];
#pragma unroll
      for (int k = 0; k < K; ++k) acc[k] = fmaf(ww, row[tx.i[b] * K + k], acc[k]);
    }
  }
#pragma unroll
  for (int k = 0; k < K; ++k) __builtin_nontemporal_store(acc[k], out + (((long long)n * K + k) * h + y) * w + x);
}

// UP2 adjoint: gz_lo [N,h,w,K] = up2^T g, g [N,K,2h,2w]; one thread per low-res pixel over the 4 x 4 high-res
// positions 2i-1 .. 2i+2 that reach it (weights up2_adj_w4; positions outside the image weigh 0 and are not read)
template <int K>
__global__ __launch_bounds__(256) void ktail_up2_bwd_kernel(const float* g, int N, int h, int w, float* gzlo) {
  const int H2 = 2 * h, W2 = 2 * w;
  const long long id = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (id >= (long long)N * h * w) return;
  const int x = (int)(id % w);
  const int y = (int)((id / w) % h);
  const int n = (int)(id / ((long long)w * h));
  const f32x4 wy = up2_adj_w4(y, h), wx = up2_adj_w4(x, w);
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const float* gp = g + ((long long)n * K + k) * H2 * W2;
    float acc = 0.f;
#pragma unroll
    for (int dy = 0; dy < 4; ++dy) {
      const int oy = 2 * y - 1 + dy;
      if (wy[dy] == 0.f) continue;  // covers oy < 0 and oy >= H2 (the edge rows' closed-form zeros)
      EUNET_DASSERT(oy >= 0 && oy < H2);
#pragma unroll
      for (int dx = 0; dx < 4; ++dx) {
        const int ox = 2 * x - 1 + dx;
        if (wx[dx] == 0.f) continue;
        EUNET_DASSERT(ox >= 0 && ox < W2);
        acc = fmaf(wy[dy] * wx[dx], __builtin_nontemporal_load(gp + (long long)oy * W2 + ox), acc);
      }
    }
    gzlo[id * K + k] = acc;
  }
}

// SMOOTH adjoint: gz_lo [N,h,w,K] = transpose of the replicate-edge filter applied to g [N,K,h,w]
template <int K>
__global__ __launch_bounds__(256) void ktail_smooth_bwd_kernel(const float* g, int N, int h, int w, float* gzlo) {
  const long long id = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (id >= (long long)N * h * w) return;
  const int x = (int)(id % w);
  const int y = (int)((id / w) % h);
  const int n = (int)(id / ((long long)w * h));
  const Tap3 ty = smooth_adj_taps(y, h), tx = smooth_adj_taps(x, w);
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const float* gp = g + ((long long)n * K + k) * h * w;
    float acc = 0.f;
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
      for (int b = 0; b < 3; ++b)  // a zero-weight tap's index is clamped into the image: read, weighted 0
        acc = fmaf(ty.w[a] * tx.w[b], gp[(long long)ty.i[a] * w + tx.i[b]], acc);
    gzlo[id * K + k] = acc;
  }
}

#define KTAIL_LAUNCH(kern, total, ARGS)                                              \
  do {                                                                               \
    const unsigned grid = (unsigned)(((total) + 255) / 256);                         \
    if (k == 1) kern<1><<<grid, 256, 0, (hipStream_t)stream>>> ARGS;                 \
    else if (k == 2) kern<2><<<grid, 256, 0, (hipStream_t)stream>>> ARGS;            \
    else kern<3><<<grid, 256, 0, (hipStream_t)stream>>> ARGS;                        \
  } while (0)

bool ktail_shape_ok(int n, int h, int w, int k) {
  // the grid of one thread per high-res pixel must fit 2^31 - 1 blocks of 256
  return n > 0 && h > 0 && w > 0 && k >= 1 && k <= 3 && (long long)n * h * w * 4 <= (1ll << 38);
}

}  // namespace

extern "C" {

int eunet_ktail_fwd(int mode, const float* z_lo, int n, int h, int w, int k, float* out, void* stream) {
  EUNET_REQUIRE(z_lo && out && ktail_shape_ok(n, h, w, k), "ktail_fwd: bad args (K must be 1..3)");
  EUNET_REQUIRE(mode == EUNET_KTAIL_UP2 || mode == EUNET_KTAIL_SMOOTH, "ktail_fwd: unknown mode %d", mode);
  const long long lo = (long long)n * h * w;
  if (mode == EUNET_KTAIL_UP2)
    KTAIL_LAUNCH(ktail_up2_fwd_kernel, 4 * lo, (z_lo, n, h, w, out));
  else
    KTAIL_LAUNCH(ktail_smooth_fwd_kernel, lo, (z_lo, n, h, w, out));
  EUNET_LAUNCH_CHECK("ktail_fwd");
  return EUNET_OK;
}

int eunet_ktail_bwd(int mode, const float* g, int n, int h, int w, int k, float* gz_lo, void* stream) {
  EUNET_REQUIRE(g && gz_lo && ktail_shape_ok(n, h, w, k), "ktail_bwd: bad args (K must be 1..3)");
  EUNET_REQUIRE(mode == EUNET_KTAIL_UP2 || mode == EUNET_KTAIL_SMOOTH, "ktail_bwd: unknown mode %d", mode);
  const long long lo = (long long)n * h * w;
  if (mode == EUNET_KTAIL_UP2)
    KTAIL_LAUNCH(ktail_up2_bwd_kernel, lo, (g, n, h, w, gz_lo));
  else
    KTAIL_LAUNCH(ktail_smooth_bwd_kernel, lo, (g, n, h, w, gz_lo));
  EUNET_LAUNCH_CHECK("ktail_bwd");
  return EUNET_OK;
}

}  // extern "C"
