// Overlap-tile inference: cutting an image into network-sized tiles and blending the tile outputs back
// into one probability map (include/eunet.h, "overlap-tile inference"; eunet/tiling.py is the geometry,
// tests/_tiling_ref.py its plain-loop restatement).  No reference line: the reference only resizes down.
//
// Both kernels are pure streaming, one pass, 16 bytes per lane wherever the addresses allow:
//   tile_gather  reads each image element once per tile that covers it (area inflation x 4 bytes) through
//                the reflect index and writes N C th tw floats; rows of a tile are contiguous runs of the
//                image row, so consecutive lanes read consecutive 16-byte units.
//   tile_blend   is organised by SOURCE position: a lane owns 4 consecutive columns of the padded image
//                that start on a multiple of 4.  Tile origins and extents are multiples of 32 and the crop
//                margin a multiple of 16, so the 4 columns lie in the same tiles at a 16-byte aligned
//                tile-local offset; the lane walks the covering tiles in increasing tile number, reads K
//                float4 per tile and writes K float4 (scalars at a ragged right edge or an unaligned w).
//                The flips mirror the destination index only.  No atomics, no weight-sum buffer.
// The geometry comes by value; every offset is 64-bit (N K th tw and C h w may pass 2^31).
#include "common.h"

EUNET_DEBUG_UNIT(tiling)

namespace {

constexpr int NT = 256;

struct Geom {
  int h, w, hp, wp;  // image, padded image (next multiples of 32)
  int th, tw;        // tile extents
  int sy, sx;        // strides
  int ny, nx;        // tile counts
};

__host__ __device__ inline int axis_count(int L, int e, int S) { return L <= e ? 1 : (L - e + S - 1) / S + 1; }
__device__ __forceinline__ int axis_origin(int i, int L, int e, int S) { return min(i * S, L - e); }
// the first tile index along an axis whose tile can reach position p: tiles i with i S + e <= p end before it
// (their origins are not clamped, since i S + e <= p < L)
__device__ __forceinline__ int first_cover(int p, int e, int S) { return p >= e ? (p - e) / S + 1 : 0; }
// F.pad(mode="reflect") to the bottom / right: position r >= n reads 2 (n - 1) - r
__device__ __forceinline__ int reflect(int r, int n) { return r < n ? r : 2 * (n - 1) - r; }

__global__ __launch_bounds__(NT) void tile_gather_kernel(const float* __restrict__ img, int C, Geom g, int first,
                                                         int count, int vec_in, float* __restrict__ tiles) {
  const int q4 = g.tw >> 2;
  const long long total = (long long)count * C * g.th * q4;
  for (long long id = (long long)blockIdx.x * NT + threadIdx.x; id < total; id += (long long)gridDim.x * NT) {
    const int q = (int)(id % q4);
    long long r = id / q4;
    const int ty = (int)(r % g.th);
    r /= g.th;
    const int c = (int)(r % C);
    const int n = first + (int)(r / C);
    const int oy = axis_origin(n / g.nx, g.hp, g.th, g.sy), ox = axis_origin(n % g.nx, g.wp, g.tw, g.sx);
    const int ry = reflect(oy + ty, g.h), x0 = ox + 4 * q;
    EUNET_DASSERT(n >= 0 && n < g.ny * g.nx && oy >= 0 && oy + g.th <= g.hp && ox >= 0 && ox + g.tw <= g.wp);
    EUNET_DASSERT(ry >= 0 && ry < g.h && x0 >= 0 && x0 + 3 < g.wp);
    const float* row = img + ((long long)c * g.h + ry) * g.w;
    float4 v;
    if (vec_in && x0 + 3 < g.w) {
      v = *reinterpret_cast<const float4*>(row + x0);
    } else {
      const int a = reflect(x0, g.w), b = reflect(x0 + 1, g.w), d = reflect(x0 + 2, g.w), e = reflect(x0 + 3, g.w);
      EUNET_DASSERT(a >= 0 && a < g.w && b >= 0 && b < g.w && d >= 0 && d < g.w && e >= 0 && e < g.w);
      v = make_float4(row[a], row[b], row[d], row[e]);
    }
    *reinterpret_cast<float4*>(tiles + id * 4) = v;
  }
}

// weight of tile-local position t of a tile at origin o (extent e) along an axis of padded length L
template <int MODE>
__device__ __forceinline__ float axis_weight(int t, int o, int e, int L, int margin, const float* tab) {
  if (MODE == EUNET_TILE_CROP) return (t >= (o > 0 ? margin : 0) && t < e - (o + e < L ? margin : 0)) ? 1.f : 0.f;
  if (MODE == EUNET_TILE_GAUSSIAN) return tab[t];
  return 1.f;
}

// act(v)[k]: the softmax over K exactly as softmax_crop_kernel forms it, the sigmoid as sigmoid_crop_kernel
template <int K, int ACT>
__device__ __forceinline__ void activate(float (&v)[K]) {
  if (ACT == EUNET_TILE_ACT_SOFTMAX) {
    float m = -INFINITY, sum = 0.f;
#pragma unroll
    for (int k = 0; k < K; ++k) m = fmaxf(m, v[k]);
#pragma unroll
    for (int k = 0; k < K; ++k) {
      v[k] = expf(v[k] - m);
      sum += v[k];
    }
#pragma unroll
    for (int k = 0; k < K; ++k) v[k] = v[k] / sum;
  } else if (ACT == EUNET_TILE_ACT_SIGMOID) {
#pragma unroll
    for (int k = 0; k < K; ++k) {
      const float e = expf(-fabsf(v[k]));
      const float r = 1.f / (1.f + e);
      v[k] = v[k] >= 0.f ? r : e * r;
    }
  }
}

template <int K, int ACT, int MODE>
__global__ __launch_bounds__(NT) void tile_blend_kernel(const float* __restrict__ logits, Geom g, int margin,
                                                        const float* __restrict__ wy_tab,
                                                        const float* __restrict__ wx_tab, int flip_h, int flip_w,
                                                        int vec_out, float* __restrict__ probs) {
  const int G = (g.w + 3) >> 2;
  const long long total = (long long)g.h * G, plane = (long long)g.th * g.tw, hw = (long long)g.h * g.w;
  for (long long id = (long long)blockIdx.x * NT + threadIdx.x; id < total; id += (long long)gridDim.x * NT) {
    const int sx0 = (int)(id % G) * 4, sy = (int)(id / G);
    float num[K][4], den[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int k = 0; k < K; ++k)
#pragma unroll
      for (int j = 0; j < 4; ++j) num[k][j] = 0.f;
    for (int iy = first_cover(sy, g.th, g.sy); iy < g.ny; ++iy) {
      const int oy = axis_origin(iy, g.hp, g.th, g.sy);
      if (oy > sy) break;
      const int ty = sy - oy;
      EUNET_DASSERT(ty >= 0 && ty < g.th);
      const float wy = axis_weight<MODE>(ty, oy, g.th, g.hp, margin, wy_tab);
      if (MODE == EUNET_TILE_CROP && wy == 0.f) continue;
      for (int ix = first_cover(sx0, g.tw, g.sx); ix < g.nx; ++ix) {
        const int ox = axis_origin(ix, g.wp, g.tw, g.sx);
        if (ox > sx0) break;
        const int tx = sx0 - ox;
        EUNET_DASSERT(tx >= 0 && tx + 3 < g.tw && (tx & 3) == 0);
        float wgt[4];
        if (MODE == EUNET_TILE_GAUSSIAN) {
          const float4 t4 = *reinterpret_cast<const float4*>(wx_tab + tx);
          wgt[0] = wy * t4.x; wgt[1] = wy * t4.y; wgt[2] = wy * t4.z; wgt[3] = wy * t4.w;
        } else {
#pragma unroll
          for (int j = 0; j < 4; ++j) wgt[j] = wy * axis_weight<MODE>(tx + j, ox, g.tw, g.wp, margin, nullptr);
        }
        if (MODE == EUNET_TILE_CROP && wgt[0] == 0.f && wgt[1] == 0.f && wgt[2] == 0.f && wgt[3] == 0.f) continue;
        const float* src = logits + (long long)(iy * g.nx + ix) * K * plane + (long long)ty * g.tw + tx;
        float4 v4[K];
#pragma unroll
        for (int k = 0; k < K; ++k) v4[k] = *reinterpret_cast<const float4*>(src + k * plane);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          float v[K];
#pragma unroll
          for (int k = 0; k < K; ++k) v[k] = j == 0 ? v4[k].x : j == 1 ? v4[k].y : j == 2 ? v4[k].z : v4[k].w;
          activate<K, ACT>(v);
#pragma unroll
          for (int k = 0; k < K; ++k) num[k][j] += wgt[j] * v[k];
          den[j] += wgt[j];
        }
      }
    }
    const int dy = flip_h ? g.h - 1 - sy : sy;
    EUNET_DASSERT(dy >= 0 && dy < g.h);
    float* orow = probs + (long long)dy * g.w;
    if (vec_out && sx0 + 3 < g.w) {
      const int dx0 = flip_w ? g.w - 4 - sx0 : sx0;
      EUNET_DASSERT(dx0 >= 0 && dx0 + 3 < g.w && (dx0 & 3) == 0);
#pragma unroll
      for (int k = 0; k < K; ++k) {
        const float a = num[k][0] / den[0], b = num[k][1] / den[1], c = num[k][2] / den[2], d = num[k][3] / den[3];
        *reinterpret_cast<float4*>(orow + k * hw + dx0) = flip_w ? make_float4(d, c, b, a) : make_float4(a, b, c, d);
      }
    } else {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (sx0 + j >= g.w) continue;
        const int dx = flip_w ? g.w - 1 - (sx0 + j) : sx0 + j;
        EUNET_DASSERT(dx >= 0 && dx < g.w);
#pragma unroll
        for (int k = 0; k < K; ++k) orow[k * hw + dx] = num[k][j] / den[j];
      }
    }
  }
}

inline unsigned grid_for(long long n) {
  const long long b = (n + NT - 1) / NT;
  return (unsigned)(b < 4096 ? (b > 0 ? b : 1) : 4096);
}

inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// the shared geometry checks; on success fills g (counts included)
int check_geom(const char* name, int h, int w, int hp, int wp, int th, int tw, int sy, int sx, Geom* g) {
  EUNET_REQUIRE(h > 0 && w > 0, "%s: the image must be at least 1 x 1 (got %d x %d)", name, h, w);
  EUNET_REQUIRE(hp == (h + 31) / 32 * 32 && wp == (w + 31) / 32 * 32,
                "%s: hp x wp must be h x w rounded up to multiples of 32 (got %d x %d for %d x %d)", name, hp, wp, h,
                w);
  EUNET_REQUIRE(hp - h < h && wp - w < w, "%s: the reflect padding must be smaller than the dimension (%d x %d)",
                name, h, w);
  EUNET_REQUIRE(th > 0 && tw > 0 && th % 32 == 0 && tw % 32 == 0 && th <= hp && tw <= wp,
                "%s: tile extents must be multiples of 32 inside the padded image (got %d x %d in %d x %d)", name, th,
                tw, hp, wp);
  EUNET_REQUIRE(sy > 0 && sx > 0 && sy % 32 == 0 && sx % 32 == 0, "%s: strides must be positive multiples of 32 "
                "(got %d, %d)", name, sy, sx);
  *g = Geom{h, w, hp, wp, th, tw, sy, sx, axis_count(hp, th, sy), axis_count(wp, tw, sx)};
  EUNET_REQUIRE((long long)g->ny * g->nx < (1ll << 31), "%s: too many tiles", name);
  return EUNET_OK;
}

template <int K, int ACT>
void launch_blend(int mode, unsigned grid, hipStream_t s, const float* logits, const Geom& g, int margin,
                  const float* wy, const float* wx, int flip_h, int flip_w, int vec_out, float* probs) {
  if (mode == EUNET_TILE_CROP)
    tile_blend_kernel<K, ACT, EUNET_TILE_CROP><<<grid, NT, 0, s>>>(logits, g, margin, wy, wx, flip_h, flip_w, vec_out,
                                                                    probs);
  else if (mode == EUNET_TILE_CONSTANT)
    tile_blend_kernel<K, ACT, EUNET_TILE_CONSTANT><<<grid, NT, 0, s>>>(logits, g, margin, wy, wx, flip_h, flip_w,
                                                                        vec_out, probs);
  else
    tile_blend_kernel<K, ACT, EUNET_TILE_GAUSSIAN><<<grid, NT, 0, s>>>(logits, g, margin, wy, wx, flip_h, flip_w,
                                                                        vec_out, probs);
}

template <int K>
void launch_blend_k(int act, int mode, unsigned grid, hipStream_t s, const float* logits, const Geom& g, int margin,
                    const float* wy, const float* wx, int flip_h, int flip_w, int vec_out, float* probs) {
  if (act == EUNET_TILE_ACT_SOFTMAX)
    launch_blend<K, EUNET_TILE_ACT_SOFTMAX>(mode, grid, s, logits, g, margin, wy, wx, flip_h, flip_w, vec_out, probs);
  else if (act == EUNET_TILE_ACT_SIGMOID)
    launch_blend<K, EUNET_TILE_ACT_SIGMOID>(mode, grid, s, logits, g, margin, wy, wx, flip_h, flip_w, vec_out, probs);
  else
    launch_blend<K, EUNET_TILE_ACT_NONE>(mode, grid, s, logits, g, margin, wy, wx, flip_h, flip_w, vec_out, probs);
}

}  // namespace

extern "C" {

int eunet_tile_gather(const float* image, int c, int h, int w, int hp, int wp, int th, int tw, int sy, int sx,
                      int first, int count, float* tiles, void* stream) {
  EUNET_REQUIRE(image && tiles, "tile_gather: null pointer");
  EUNET_REQUIRE(c >= 1 && c <= 4, "tile_gather: C must be 1..4 (got %d)", c);
  Geom g;
  const int rc = check_geom("tile_gather", h, w, hp, wp, th, tw, sy, sx, &g);
  if (rc) return rc;
  EUNET_REQUIRE(first >= 0 && count > 0 && (long long)first + count <= (long long)g.ny * g.nx,
                "tile_gather: tiles %d .. %d are not inside the plan's %d x %d tiles", first, first + count - 1, g.ny,
                g.nx);
  EUNET_REQUIRE(aligned16(tiles), "tile_gather: tiles must be 16-byte aligned");
  const int vec_in = (w % 4 == 0 && aligned16(image)) ? 1 : 0;
  const long long total = (long long)count * c * th * (tw / 4);
  tile_gather_kernel<<<grid_for(total), NT, 0, (hipStream_t)stream>>>(image, c, g, first, count, vec_in, tiles);
  EUNET_LAUNCH_CHECK("tile_gather");
  return EUNET_OK;
}

int eunet_tile_blend(const float* logits, int k, int h, int w, int hp, int wp, int th, int tw, int sy, int sx,
                     int mode, int margin, const float* wy, const float* wx, int activation, int flip_h, int flip_w,
                     float* probs, void* stream) {
  EUNET_REQUIRE(logits && probs, "tile_blend: null pointer");
  EUNET_REQUIRE(k >= 1 && k <= 3, "tile_blend: K must be 1..3 (got %d)", k);
  Geom g;
  const int rc = check_geom("tile_blend", h, w, hp, wp, th, tw, sy, sx, &g);
  if (rc) return rc;
  EUNET_REQUIRE(mode == EUNET_TILE_CROP || mode == EUNET_TILE_CONSTANT || mode == EUNET_TILE_GAUSSIAN,
                "tile_blend: unknown blend mode %d", mode);
  EUNET_REQUIRE(activation == EUNET_TILE_ACT_NONE || activation == EUNET_TILE_ACT_SOFTMAX ||
                    activation == EUNET_TILE_ACT_SIGMOID,
                "tile_blend: unknown activation %d", activation);
  if (mode == EUNET_TILE_CROP) {
    EUNET_REQUIRE(margin >= 0 && margin % 16 == 0, "tile_blend: margin must be a non-negative multiple of 16 (got %d)",
                  margin);
    // the cores [o + margin, o + e - margin) of consecutive tiles must abut or overlap: full coverage
    EUNET_REQUIRE((g.ny == 1 || sy + 2 * margin <= th) && (g.nx == 1 || sx + 2 * margin <= tw),
                  "tile_blend: stride + 2 margin exceeds the tile: the cropped cores leave pixels uncovered");
  } else {
    EUNET_REQUIRE((g.ny == 1 || sy <= th) && (g.nx == 1 || sx <= tw),
                  "tile_blend: a stride exceeds the tile: pixels are left uncovered");
  }
  if (mode == EUNET_TILE_GAUSSIAN)
    EUNET_REQUIRE(wy && wx && aligned16(wx), "tile_blend: the gaussian mode needs its weight tables wy [th], wx [tw] "
                  "(wx 16-byte aligned)");
  EUNET_REQUIRE(aligned16(logits), "tile_blend: logits must be 16-byte aligned");
  const int vec_out = (w % 4 == 0 && aligned16(probs)) ? 1 : 0;
  const unsigned grid = grid_for((long long)h * ((w + 3) / 4));
  hipStream_t s = (hipStream_t)stream;
  if (k == 1) launch_blend_k<1>(activation, mode, grid, s, logits, g, margin, wy, wx, flip_h, flip_w, vec_out, probs);
  else if (k == 2) launch_blend_k<2>(activation, mode, grid, s, logits, g, margin, wy, wx, flip_h, flip_w, vec_out, probs);
  else launch_blend_k<3>(activation, mode, grid, s, logits, g, margin, wy, wx, flip_h, flip_w, vec_out, probs);
  EUNET_LAUNCH_CHECK("tile_blend");
  return EUNET_OK;
}

}  // extern "C"
