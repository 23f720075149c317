// Elastic deformation and affine warp of the device data path (include/eunet.h holds the definitions; no
// reference line to cite: the reference's augmentations are photometric or a mirror).  The deformation is the
// one of Ronneberger et al., "U-Net" (2015), §3.1: random displacements on a coarse control grid, interpolated
// bicubically to one displacement per pixel, applied to the image and to its labels together.
//
// warp_grid_kernel: one 256-thread block per output row.  The control points (at most 16 x 16 x 2) are first
// interpolated along y into one LDS row of 2 x gw values (threads 0 .. 2 gw - 1, four taps each), then every
// pixel of the row takes its four taps along x from that row and adds the affine part; one 8-byte store per
// pixel, 512 contiguous bytes per wave.  The position of a pixel between control points is computed in
// integers (x (gw - 1) = q (w - 1) + r: cell q, fraction r / (w - 1) rounded once), so the cubic weights see
// the fraction at fp32's full relative precision at every image size.
//
// warp_u8_kernel<C>: one block per 256 consecutive pixels of the flat HWC output, one pixel per lane: an 8-byte
// read of the map, 4 C byte gathers, and the block's 256 C bytes leave through an LDS tile as 16 C 16-byte
// stores (rows of C = 3 bytes need no alignment of their own: the block's first byte is 256 C bytes into the
// buffer).  The ragged last block and an unaligned buffer take byte stores.  A wave's gather then reads 64
// neighbouring source pixels; with four pixels per lane (measured first) it read four times that span per
// instruction and took 1.9 times as long at a 20 degree rotation (33 against 18 us at 1024^2 x 3).  What is
// left depends on the rotation, because a wave's 64 pixels of one output row cross more source rows the
// steeper the map (10 us at 0, 18 at 20, 32 at 90 degrees): a two-dimensional wave footprint would level that.
//
// warp_ids_kernel (int64) and warp_stack_kernel (uint8): the map is turned into one source offset per pixel
// (-1: fill) once and then serves every plane of the block's chunk (blockIdx.y): 16-byte stores in both, two
// pixels per lane for int64, one pixel per lane and an LDS transpose for uint8 (at the kernel).  A plane size
// that is not a multiple of 16 bytes misaligns the later planes: element stores then.
//
// All three are bound by memory traffic and by the gather instructions' issue rate, not by arithmetic: the
// index arithmetic after the single rintf is integer.
#include <math.h>

#include "common.h"

EUNET_DEBUG_UNIT(warp)

namespace {
constexpr int NT = 256;
constexpr int GMAX = 16;            // control points per axis: 2 .. GMAX
constexpr int MAX_SIDE = 1 << 20;   // image and map sides; coordinates are clamped to +-MAX_SIDE
constexpr int PCHUNK = 32;          // int64 label planes per block
constexpr int SGROUP = 16;          // uint8 planes per pass through the LDS tile: NT / 16 lanes take one plane's 256 pixels
constexpr int SCHUNK = 64;          // uint8 planes per block: the map is read once per pixel and SCHUNK planes
static_assert(SGROUP * 16 == NT, "one 16-byte store per lane empties the tile");
constexpr float CUBIC_A = -0.75f;   // the cubic-convolution kernel of F.interpolate(mode="bicubic")

// weights of the taps floor(u) - 1 .. floor(u) + 2 at fraction t = u - floor(u), s = 1 - t.  The two cubics
//   |d| <= 1: (A + 2) d^3 - (A + 3) d^2 + 1 = (1 - d) (1 + d - (A + 2) d^2)
//   |d| >= 1:  A d^3 - 5 A d^2 + 8 A d - 4 A = A (d - 1) (d - 2)^2
// are evaluated in their factored forms: no cancellation, so every weight carries a few ulps of its own
// size (Horner's form leaves a few ulps of 8 |A| = 6 on weights below 0.15, which shows once the
// displacements are large against the image)
__device__ __forceinline__ void cubic_weights(float t, float (&w)[4]) {
  constexpr float B = CUBIC_A + 2.f;
  const float s = 1.f - t;
  w[0] = CUBIC_A * t * s * s;
  w[1] = s * (1.f + t - B * t * t);
  w[2] = t * (1.f + s - B * s * s);
  w[3] = CUBIC_A * s * t * t;
}

// u = x (g - 1) / (n - 1) (align_corners=True; 0 when n == 1) as cell and fraction
__device__ __forceinline__ void ctrl_pos(int x, int n, int g, int& cell, float& t) {
  if (n == 1) {
    cell = 0;
    t = 0.f;
    return;
  }
  const int num = x * (g - 1);  // < 2^20 * 15
  cell = num / (n - 1);
  t = (float)(num - cell * (n - 1)) / (float)(n - 1);
}

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

__global__ __launch_bounds__(NT) void warp_grid_kernel(const float* ctrl, int gh, int gw, float m00, float m01, float m02,
                                                       float m10, float m11, float m12, int h, int w, float2* grid) {
  __shared__ float rowc[2 * GMAX];  // [plane][gw]: the control grid interpolated to this row
  const int y = blockIdx.x, tid = threadIdx.x;
  if (tid < 2 * gw) {
    const int p = tid / gw, j = tid - p * gw;
    int cell;
    float t, wy[4];
    ctrl_pos(y, h, gh, cell, t);
    cubic_weights(t, wy);
    float acc = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int iy = clampi(cell - 1 + i, 0, gh - 1);
      EUNET_DASSERT(iy >= 0 && iy < gh && j >= 0 && j < gw && p >= 0 && p < 2);
      acc = fmaf(wy[i], ctrl[(p * gh + iy) * gw + j], acc);
    }
    rowc[p * gw + j] = acc;
  }
  __syncthreads();
  const float ay = fmaf(m01, (float)y, m02), by = fmaf(m11, (float)y, m12);
  for (int x = tid; x < w; x += NT) {
    int cell;
    float t, wx[4];
    ctrl_pos(x, w, gw, cell, t);
    cubic_weights(t, wx);
    float dx = 0.f, dy = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int ix = clampi(cell - 1 + i, 0, gw - 1);
      EUNET_DASSERT(ix >= 0 && ix < gw);
      dx = fmaf(wx[i], rowc[ix], dx);
      dy = fmaf(wx[i], rowc[gw + ix], dy);
    }
    grid[(long long)y * w + x] = make_float2(fmaf(m00, (float)x, ay) + dx, fmaf(m10, (float)x, by) + dy);
  }
}

// (sx, sy) -> 1/32-pixel fixed point; false: a non-finite coordinate (the pixel is `fill`)
__device__ __forceinline__ bool quantise(float2 s, int& qx, int& qy) {
  if (!isfinite(s.x) || !isfinite(s.y)) return false;
  const float L = (float)MAX_SIDE;
  qx = (int)rintf(fminf(fmaxf(s.x, -L), L) * 32.f);  // exact product, round-half-even
  qy = (int)rintf(fminf(fmaxf(s.y, -L), L) * 32.f);
  return true;
}

// index i of an axis of n pixels under the border rule; -1: outside (constant border)
__device__ __forceinline__ int border_index(int i, int n, int border) {
  if (border == 0) return (i >= 0 && i < n) ? i : -1;
  if (n == 1) return 0;
  const int p = 2 * (n - 1);
  int r = i % p;
  if (r < 0) r += p;
  if (r >= n) r = p - r;
  EUNET_DASSERT(r >= 0 && r < n);
  return r;
}

template <int C>
__device__ __forceinline__ void sample_bilinear(const uint8_t* src, int hi, int wi, float2 s, int border, int fill,
                                                uint8_t* out) {
  int qx, qy;
  if (!quantise(s, qx, qy)) {
#pragma unroll
    for (int ch = 0; ch < C; ++ch) out[ch] = (uint8_t)fill;
    return;
  }
  const int ix = qx >> 5, fx = qx & 31, iy = qy >> 5, fy = qy & 31;
  const int x0 = border_index(ix, wi, border), x1 = border_index(ix + 1, wi, border);
  const int y0 = border_index(iy, hi, border), y1 = border_index(iy + 1, hi, border);
  const int w00 = (32 - fx) * (32 - fy), w01 = fx * (32 - fy), w10 = (32 - fx) * fy, w11 = fx * fy;
  const int o00 = (x0 < 0 || y0 < 0) ? -1 : (y0 * wi + x0) * C, o01 = (x1 < 0 || y0 < 0) ? -1 : (y0 * wi + x1) * C;
  const int o10 = (x0 < 0 || y1 < 0) ? -1 : (y1 * wi + x0) * C, o11 = (x1 < 0 || y1 < 0) ? -1 : (y1 * wi + x1) * C;
  EUNET_DASSERT(o00 < hi * wi * C && o01 < hi * wi * C && o10 < hi * wi * C && o11 < hi * wi * C);
#pragma unroll
  for (int ch = 0; ch < C; ++ch) {
    const int p00 = o00 < 0 ? fill : (int)src[o00 + ch], p01 = o01 < 0 ? fill : (int)src[o01 + ch];
    const int p10 = o10 < 0 ? fill : (int)src[o10 + ch], p11 = o11 < 0 ? fill : (int)src[o11 + ch];
    out[ch] = (uint8_t)((w00 * p00 + w01 * p01 + w10 * p10 + w11 * p11 + 512) >> 10);
  }
}

// One pixel per lane, 256 consecutive pixels of the flat HWC output per block: a wave's gather of one tap and
// channel reads 64 neighbouring source pixels.  The 256 C bytes go through LDS and leave as 16 C 16-byte stores.
template <int C>
__global__ __launch_bounds__(NT) void warp_u8_kernel(const uint8_t* src, int hi, int wi, const float2* grid,
                                                     long long total, int border, int fill, uint8_t* dst, int vec) {
  __shared__ __attribute__((aligned(16))) uint8_t tile[NT * C];
  const long long nblk = (total + NT - 1) / NT;
  const int t = threadIdx.x;
  for (long long b = blockIdx.x; b < nblk; b += gridDim.x) {
    const long long o = b * NT;
    const bool live = o + t < total, full = vec && o + NT <= total;  // full is block-uniform
    uint8_t v[C];
    if (live) sample_bilinear<C>(src, hi, wi, grid[o + t], border, fill, v);
    if (full) {
#pragma unroll
      for (int ch = 0; ch < C; ++ch) tile[t * C + ch] = v[ch];
      __syncthreads();
      if (t < 16 * C) {
        EUNET_DASSERT((o * C + t * 16 + 16) <= total * C);
        *(uint4*)(dst + o * C + t * 16) = *(const uint4*)&tile[t * 16];
      }
      __syncthreads();
    } else if (live) {
#pragma unroll
      for (int ch = 0; ch < C; ++ch) dst[(o + t) * C + ch] = v[ch];
    }
  }
}

// (y, x) of the output -> offset into a source plane, -1: fill
__device__ __forceinline__ int nearest_offset(const float2* grid, int y, int x, int ho, int wo, int hi, int wi, int border,
                                              int flip_h, int flip_v) {
  const int gy = flip_v ? ho - 1 - y : y, gx = flip_h ? wo - 1 - x : x;
  EUNET_DASSERT(gy >= 0 && gy < ho && gx >= 0 && gx < wo);
  int qx, qy;
  if (!quantise(grid[(long long)gy * wo + gx], qx, qy)) return -1;
  const int bx = border_index((qx + 16) >> 5, wi, border), by = border_index((qy + 16) >> 5, hi, border);
  if (bx < 0 || by < 0) return -1;
  EUNET_DASSERT(bx < wi && by < hi);
  return by * wi + bx;
}

// The int64 map(s): every thread takes two consecutive pixels (one 16-byte store) of each plane of its chunk.
__global__ __launch_bounds__(NT) void warp_ids_kernel(const int64_t* src, int planes, int hi, int wi, const float2* grid,
                                                      int ho, int wo, int border, int64_t fill, int flip_h, int flip_v,
                                                      int64_t* dst, int vec) {
  const long long total = (long long)ho * wo, groups = (total + 1) / 2, splane = (long long)hi * wi;
  const int p0 = blockIdx.y * PCHUNK, p1 = p0 + PCHUNK < planes ? p0 + PCHUNK : planes;
  for (long long g = (long long)blockIdx.x * NT + threadIdx.x; g < groups; g += (long long)gridDim.x * NT) {
    const long long o = g * 2;
    const bool pair = o + 1 < total;
    const int y0 = (int)(o / wo), x0 = (int)(o - (long long)y0 * wo);
    const int x1 = x0 + 1 == wo ? 0 : x0 + 1, y1 = x0 + 1 == wo ? y0 + 1 : y0;
    const int off0 = nearest_offset(grid, y0, x0, ho, wo, hi, wi, border, flip_h, flip_v);
    const int off1 = pair ? nearest_offset(grid, y1, x1, ho, wo, hi, wi, border, flip_h, flip_v) : -1;
    for (int p = p0; p < p1; ++p) {
      const int64_t* sp = src + (long long)p * splane;
      int64_t* dp = dst + (long long)p * total + o;
      const int64_t v0 = off0 < 0 ? fill : sp[off0], v1 = off1 < 0 ? fill : sp[off1];
      if (pair && vec) {
        *(longlong2*)dp = make_longlong2(v0, v1);
      } else {
        dp[0] = v0;
        if (pair) dp[1] = v1;
      }
    }
  }
}

// The uint8 stack: one block per 256 consecutive pixels and chunk of SCHUNK planes, one pixel per lane, so that
// a wave's gather of one plane reads 64 neighbouring source bytes (a few cache lines under a smooth map; with 16
// pixels per lane as above it touched sixteen times as many for the same 64 bytes, and ran at a third of the rate).
// Sixteen planes at a time go through an LDS tile [16][256] that turns the lane-per-pixel bytes into one
// 16-byte store per lane (plane tid / 16, pixels 16 (tid % 16) ..).  The ragged last block and planes that are
// not 16-byte aligned store their bytes straight from the registers.
__global__ __launch_bounds__(NT) void warp_stack_kernel(const uint8_t* src, int planes, int hi, int wi, const float2* grid,
                                                        int ho, int wo, int border, uint8_t fill, int flip_h, int flip_v,
                                                        uint8_t* dst, int vec) {
  __shared__ __attribute__((aligned(16))) uint8_t tile[SGROUP][NT];
  const long long total = (long long)ho * wo, splane = (long long)hi * wi, nblk = (total + NT - 1) / NT;
  const int p0 = blockIdx.y * SCHUNK, p1 = p0 + SCHUNK < planes ? p0 + SCHUNK : planes;
  const int t = threadIdx.x;
  for (long long b = blockIdx.x; b < nblk; b += gridDim.x) {
    const long long o = b * NT;
    const bool live = o + t < total, full = vec && o + NT <= total;  // full is block-uniform
    int off = -1;
    if (live) {
      const int y = (int)((o + t) / wo), x = (int)(o + t - (long long)y * wo);
      off = nearest_offset(grid, y, x, ho, wo, hi, wi, border, flip_h, flip_v);
    }
    for (int pb = p0; pb < p1; pb += SGROUP) {
      const int np = p1 - pb < SGROUP ? p1 - pb : SGROUP;
      uint8_t v[SGROUP];
#pragma unroll
      for (int k = 0; k < SGROUP; ++k) {
        EUNET_DASSERT(off < splane);
        v[k] = (k < np && off >= 0) ? src[(long long)(pb + k) * splane + off] : fill;
      }
      if (full) {
#pragma unroll
        for (int k = 0; k < SGROUP; ++k) tile[k][t] = v[k];
        __syncthreads();
        const int k = t >> 4, c = (t & 15) * 16;
        if (k < np) {
          EUNET_DASSERT(pb + k < planes && o + c + 16 <= total);
          *(uint4*)(dst + (long long)(pb + k) * total + o + c) = *(const uint4*)&tile[k][c];
        }
        __syncthreads();
      } else if (live) {
#pragma unroll
        for (int k = 0; k < SGROUP; ++k)
          if (k < np) dst[(long long)(pb + k) * total + o + t] = v[k];
      }
    }
  }
}

unsigned blocks_for(long long items) {
  const long long b = (items + NT - 1) / NT;
  return (unsigned)(b > 65535 ? 65535 : (b < 1 ? 1 : b));
}

bool aligned(const void* p, size_t a) { return ((uintptr_t)p & (a - 1)) == 0; }

bool sides_ok(int h, int w) { return h >= 1 && w >= 1 && h <= MAX_SIDE && w <= MAX_SIDE; }
}  // namespace

extern "C" {

int eunet_warp_grid(const float* ctrl, int gh, int gw, const double* m, int h, int w, float* grid, void* stream) {
  EUNET_REQUIRE(ctrl && grid && aligned(grid, 8), "warp_grid: bad args (ctrl, grid non-null; grid 8-byte aligned)");
  EUNET_REQUIRE(gh >= 2 && gh <= GMAX && gw >= 2 && gw <= GMAX, "warp_grid: control grid %d x %d outside 2..%d", gh, gw,
                GMAX);
  EUNET_REQUIRE(sides_ok(h, w), "warp_grid: size %d x %d outside 1..%d", h, w, MAX_SIDE);
  float f[6] = {1.f, 0.f, 0.f, 0.f, 1.f, 0.f};
  for (int i = 0; m && i < 6; ++i) {
    EUNET_REQUIRE(m[i] == m[i] && m[i] > -3e38 && m[i] < 3e38, "warp_grid: matrix entry %d is not a finite float", i);
    f[i] = (float)m[i];
  }
  warp_grid_kernel<<<(unsigned)h, NT, 0, (hipStream_t)stream>>>(ctrl, gh, gw, f[0], f[1], f[2], f[3], f[4], f[5], h, w,
                                                               (float2*)grid);
  EUNET_LAUNCH_CHECK("warp_grid");
  return EUNET_OK;
}

int eunet_warp_u8(const uint8_t* src, int hi, int wi, int c, const float* grid, int ho, int wo, int border, int fill,
                  uint8_t* dst, void* stream) {
  EUNET_REQUIRE(src && grid && dst && src != dst && aligned(grid, 8),
                "warp_u8: bad args (src, grid, dst non-null; not in place; grid 8-byte aligned)");
  EUNET_REQUIRE(c >= 1 && c <= 4 && sides_ok(hi, wi) && sides_ok(ho, wo) && (long long)hi * wi * c < (1ll << 31),
                "warp_u8: needs 1 <= c <= 4, sides in 1..%d and a source below 2^31 bytes", MAX_SIDE);
  EUNET_REQUIRE((border == EUNET_WARP_CONSTANT || border == EUNET_WARP_REFLECT101) && fill >= 0 && fill <= 255,
                "warp_u8: border %d is neither constant (0) nor reflect-101 (1), or fill %d outside 0..255", border, fill);
  const long long total = (long long)ho * wo;
  const float2* gr = (const float2*)grid;
  hipStream_t s = (hipStream_t)stream;
  const int vec = aligned(dst, 16);
  const long long nblk = (total + NT - 1) / NT;
  const unsigned g = (unsigned)(nblk > 65535 ? 65535 : nblk);
  if (c == 1) warp_u8_kernel<1><<<g, NT, 0, s>>>(src, hi, wi, gr, total, border, fill, dst, vec);
  else if (c == 2) warp_u8_kernel<2><<<g, NT, 0, s>>>(src, hi, wi, gr, total, border, fill, dst, vec);
  else if (c == 3) warp_u8_kernel<3><<<g, NT, 0, s>>>(src, hi, wi, gr, total, border, fill, dst, vec);
  else warp_u8_kernel<4><<<g, NT, 0, s>>>(src, hi, wi, gr, total, border, fill, dst, vec);
  EUNET_LAUNCH_CHECK("warp_u8");
  return EUNET_OK;
}

int eunet_warp_labels(const void* src, int elem_bytes, int planes, int hi, int wi, const float* grid, int ho, int wo,
                      int border, long long fill, int flip_h, int flip_v, void* dst, void* stream) {
  EUNET_REQUIRE((elem_bytes == 8 || elem_bytes == 1) && planes >= 0 && planes <= 65535 * PCHUNK,
                "warp_labels: elem_bytes %d is neither 8 (int64) nor 1 (uint8), or bad plane count %d", elem_bytes, planes);
  EUNET_REQUIRE(sides_ok(hi, wi) && sides_ok(ho, wo) && (long long)hi * wi < (1ll << 31),
                "warp_labels: sides outside 1..%d or a source plane of 2^31 pixels or more", MAX_SIDE);
  EUNET_REQUIRE((border == EUNET_WARP_CONSTANT || border == EUNET_WARP_REFLECT101) &&
                    (elem_bytes == 8 || (fill >= 0 && fill <= 255)),
                "warp_labels: border %d is neither constant (0) nor reflect-101 (1), or fill outside 0..255", border);
  if (planes == 0) return EUNET_OK;
  EUNET_REQUIRE(src && grid && dst && src != dst && aligned(grid, 8) && aligned(src, (size_t)elem_bytes) &&
                    aligned(dst, (size_t)elem_bytes),
                "warp_labels: bad args (src, grid, dst non-null and aligned to their elements; not in place)");
  const long long total = (long long)ho * wo;
  const int vec = aligned(dst, 16) && (planes == 1 || total * elem_bytes % 16 == 0);
  const float2* gr = (const float2*)grid;
  hipStream_t s = (hipStream_t)stream;
  if (elem_bytes == 8) {
    warp_ids_kernel<<<dim3(blocks_for((total + 1) / 2), (unsigned)cdiv(planes, PCHUNK)), NT, 0, s>>>(
        (const int64_t*)src, planes, hi, wi, gr, ho, wo, border, (int64_t)fill, flip_h != 0, flip_v != 0, (int64_t*)dst, vec);
  } else {
    const long long nblk = (total + NT - 1) / NT;
    warp_stack_kernel<<<dim3((unsigned)(nblk > 65535 ? 65535 : nblk), (unsigned)cdiv(planes, SCHUNK)), NT, 0, s>>>(
        (const uint8_t*)src, planes, hi, wi, gr, ho, wo, border, (uint8_t)fill, flip_h != 0, flip_v != 0, (uint8_t*)dst, vec);
  }
  EUNET_LAUNCH_CHECK("warp_labels");
  return EUNET_OK;
}

}  // extern "C"
