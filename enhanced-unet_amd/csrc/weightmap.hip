// U-Net border weight map and the separation of touching instances (include/eunet.h holds the
// definitions; no reference line to cite: the reference fills its polygons into one 0/1/2 mask and has
// neither).  The map is the per-pixel weight of Ronneberger et al., "U-Net" (2015), eq. 2, with the
// window of the definition made explicit:
//   m(x) = base(x) + [labels(x) = 0 and two ids in the window] w0 exp(-(d1 + d2)^2 / (2 sigma^2))
// d1 <= d2 the distances to the two nearest distinct instance ids among the pixels q of the same sample
// with |qx - xx| <= R and |qy - xy| <= R.
//
// border_weight_kernel: one 256-thread block per 32x32 output tile and sample.  The tile plus an R-wide
// halo of labels is staged in LDS narrowed to 32 bits ((32 + 2R)^2 words: 64 KiB at R = 48), outside the
// image as background.  While staging, the block finds out whether its region holds two distinct ids; if
// not, no pixel of the tile can have a border term and the block writes base and leaves.  Otherwise the
// block marks its candidates in a bit mask per staged row (4 words: a row has at most 128 pixels): the cell
// pixels that are not interior, i.e. not surrounded by their own id on all four sides.  The nearest pixel
// of an instance to a pixel outside it is never interior (from an interior pixel, one step towards the
// outside pixel stays in the instance and in the window and is strictly nearer), so the minimum over the
// candidates is the minimum over the instance.  Each background lane then scans its window row by row
// outwards from its own row (dy = 0, -1, +1, -2, ...), reading per row the mask words that overlap its
// window and visiting only their set bits, and keeps (d^2, id) of the two nearest distinct ids in
// integers; a row pair at |dy| with dy^2 >= the second-best d^2 ends the scan, and within a row only the
// |dx| that can still beat the second best are looked at.  Open background costs a few mask words per
// row instead of 2R + 1 labels.  Then two sqrtf and one expf.  Integer d^2 is exact, so the only roundings
// are in (d1 + d2)^2 / (2 sigma^2), the exponential and the final sum.
#include "common.h"

EUNET_DEBUG_UNIT(weightmap)

namespace {
constexpr int NT = 256;
constexpr int WT = 32;                   // output tile side; NT threads take 4 rows apart by 8 each
constexpr int WMAX_R = 48;               // (WT + 2 * 48)^2 * 4 bytes = 64 KiB of the CU's 160 KiB of LDS
constexpr int MW = 4;                    // 32-bit candidate-mask words per staged row: WT + 2 * WMAX_R = 128 bits
constexpr unsigned NONE = 0xFFFFFFFFu;   // d^2 of an empty slot

struct Near2 {
  unsigned d1, d2;  // squared distances to the nearest and the second-nearest distinct id; NONE: no such id
};

// A candidate of the staged region st (row stride S, 0 = background): a cell pixel that is not surrounded by
// its own id on all four sides; a pixel on the rim of the staged region counts as not surrounded.
__host__ __device__ inline bool candidate(const uint32_t* st, int S, int sx, int sy) {
  const uint32_t id = st[sy * S + sx];
  if (id == 0u) return false;
  if (sx == 0 || sy == 0 || sx == S - 1 || sy == S - 1) return true;
  return st[sy * S + sx - 1] != id || st[sy * S + sx + 1] != id || st[(sy - 1) * S + sx] != id ||
         st[(sy + 1) * S + sx] != id;
}

// The window scan of one background pixel at (cx, cy) of the staged region st with its candidate masks occ
// ([S][MW], bit sx of row sy set iff candidate(st, S, sx, sy)); the caller guarantees R staged words on every
// side of the pixel.  Host-callable so that a CPU build can check it against a brute-force restatement
// (tools/weightmap_scan_check.cpp).
__host__ __device__ inline Near2 two_nearest(const uint32_t* st, const uint32_t* occ, int S, int cx, int cy, int R) {
  unsigned b1 = NONE, b2 = NONE;
  uint32_t i1 = 0, i2 = 0;  // 0 never matches a candidate: candidates are non-background
  for (int a = 0; a <= R; ++a) {
    const unsigned a2 = (unsigned)(a * a);
    if (a2 >= b2) break;  // every pixel of rows +-a and beyond is at d^2 >= a2: no value can change any more
    for (int sg = 0; sg < (a ? 2 : 1); ++sg) {
      const int sy = cy + (sg ? a : -a);
      // only d^2 = a2 + dx^2 < b2 can change a value; the float root is exact to well within the +1
      int rx = R;
      if (b2 != NONE) {
        const int r = (int)sqrtf((float)(b2 - a2)) + 1;
        rx = r < R ? r : R;
      }
      const int lo = cx - rx, hi = cx + rx;  // inclusive, inside the staged row
      for (int w = lo >> 5; w <= (hi >> 5); ++w) {
        uint32_t m = occ[sy * MW + w];
        if (w == (lo >> 5)) m &= 0xFFFFFFFFu << (lo & 31);
        if (w == (hi >> 5)) m &= 0xFFFFFFFFu >> (31 - (hi & 31));
        while (m) {
          const int sx = (w << 5) + __builtin_ctz(m);
          m &= m - 1u;
          const uint32_t id = st[sy * S + sx];
          const int dx = sx - cx;
          const unsigned d = a2 + (unsigned)(dx * dx);
          if (id == i1) {
            b1 = d < b1 ? d : b1;
          } else if (id == i2) {
            if (d < b2) {
              b2 = d;
              if (b2 < b1) {
                const unsigned tb = b1;
                b1 = b2;
                b2 = tb;
                i2 = i1;
                i1 = id;
              }
            }
          } else if (d < b1) {
            b2 = b1;
            i2 = i1;
            b1 = d;
            i1 = id;
          } else if (d < b2) {
            b2 = d;
            i2 = id;
          }
        }
      }
    }
  }
  return {b1, b2};
}

__global__ __launch_bounds__(NT) void border_weight_kernel(const int64_t* labels, const int64_t* semantic, int H,
                                                           int W, float cw0, float cw1, float cw2, float w0,
                                                           float inv2s2, int R, float* out) {
  extern __shared__ __attribute__((aligned(16))) uint32_t st[];  // [S][S] labels, [S][MW] masks, two words
  const int tid = threadIdx.x;
  const int S = WT + 2 * R;
  uint32_t* occ = st + S * S;              // candidate masks per staged row
  uint32_t& s_first = occ[S * MW];         // one id of the staged region (0: none)
  uint32_t& s_multi = occ[S * MW + 1];     // 1: the staged region holds two distinct ids
  const int x0 = blockIdx.x * WT, y0 = blockIdx.y * WT;
  const long long img = (long long)blockIdx.z * H * W;
  const int64_t* lb = labels + img;
  if (tid == 0) {
    s_first = 0u;
    s_multi = 0u;
  }
  for (int i = tid; i < S * MW; i += NT) occ[i] = 0u;
  // stage; first / multi: the first id this thread met, and whether it met another one
  uint32_t first = 0u;
  bool multi = false;
  for (int i = tid; i < S * S; i += NT) {
    const int sy = i / S, sx = i - sy * S;
    const int gy = y0 - R + sy, gx = x0 - R + sx;
    uint32_t id = 0u;
    if (gy >= 0 && gy < H && gx >= 0 && gx < W) id = (uint32_t)lb[(long long)gy * W + gx];
    st[i] = id;
    if (id) {
      if (!first) first = id;
      else if (id != first) multi = true;
    }
  }
  __syncthreads();
  if (first) atomicCAS(&s_first, 0u, first);
  __syncthreads();
  if (multi || (first && first != s_first)) s_multi = 1u;
  __syncthreads();
  const bool scan = s_multi != 0u;  // block-uniform: fewer than two ids staged -> every pixel is base
  if (scan) {
    for (int i = tid; i < S * S; i += NT) {
      const int sy = i / S, sx = i - sy * S;
      if (candidate(st, S, sx, sy)) {
        EUNET_DASSERT((sx >> 5) < MW);
        atomicOr(&occ[sy * MW + (sx >> 5)], 1u << (sx & 31));
      }
    }
    __syncthreads();
  }
  const int lx = tid & (WT - 1);
#pragma unroll
  for (int j = 0; j < WT * WT / NT; ++j) {
    const int ly = (tid >> 5) + j * (NT / WT);
    const int gy = y0 + ly, gx = x0 + lx;
    if (gy >= H || gx >= W) continue;
    const long long o = img + (long long)gy * W + gx;
    float m = 1.f;
    if (semantic) {
      const int64_t sv = semantic[o];
      m = sv == 0 ? cw0 : sv == 1 ? cw1 : sv == 2 ? cw2 : 1.f;
    }
    const int c = (ly + R) * S + lx + R;
    EUNET_DASSERT(c - R * S - R >= 0 && c + R * S + R < S * S);
    if (scan && st[c] == 0u) {
      const Near2 nn = two_nearest(st, occ, S, lx + R, ly + R, R);
      if (nn.d2 != NONE) {
        const float s = sqrtf((float)nn.d1) + sqrtf((float)nn.d2);
        m += w0 * expf(-(s * s) * inv2s2);
      }
    }
    out[o] = m;
  }
}

__global__ __launch_bounds__(NT) void separate_kernel(const int64_t* labels, const int64_t* semantic, long long total,
                                                      int H, int W, int64_t* labels_out, int64_t* semantic_out) {
  for (long long id = (long long)blockIdx.x * NT + threadIdx.x; id < total; id += (long long)gridDim.x * NT) {
    const int x = (int)(id % W);
    const int y = (int)((id / W) % H);
    const long long img = id - ((long long)y * W + x);
    const int64_t v = labels[id];
    bool cut = false;
    for (int dy = -1; dy <= 1; ++dy)
      for (int dx = -1; dx <= 1; ++dx) {
        const int yy = y + dy, xx = x + dx;
        if (yy < 0 || yy >= H || xx < 0 || xx >= W) continue;
        EUNET_DASSERT(img + (long long)yy * W + xx < total);
        const int64_t u = labels[img + (long long)yy * W + xx];
        cut = cut || (u != 0 && u != v);
      }
    labels_out[id] = cut ? 0 : v;
    if (semantic_out) semantic_out[id] = cut ? 0 : semantic[id];
  }
}
}  // namespace

extern "C" {

int eunet_border_weight_map(const int64_t* labels, const int64_t* semantic, int n, int h, int w,
                            const float* class_weight, float w0, float sigma, int radius, float* out, void* stream) {
  EUNET_REQUIRE(labels && out && n > 0 && n <= 65535 && h > 0 && w > 0 && (long long)n * h * w < (1ll << 40),
                "border_weight_map: bad args (labels, out non-null; N <= 65535)");
  EUNET_REQUIRE(sigma > 0.f && sigma < 1e18f && w0 >= 0.f && w0 < 3e38f,
                "border_weight_map: needs sigma > 0 and w0 >= 0 (finite), got sigma %g, w0 %g", (double)sigma, (double)w0);
  int R = radius;
  if (R == EUNET_WMAP_RADIUS_AUTO) {
    const double r = 5.5 * (double)sigma;
    R = r > 1e6 ? 1000000 : (int)r + ((double)(int)r < r ? 1 : 0);  // ceil
  }
  EUNET_REQUIRE(R >= 1 && R <= WMAX_R, "border_weight_map: radius %d outside 1..%d (the default is ceil(5.5 sigma))", R,
                WMAX_R);
  const float cw[3] = {class_weight ? class_weight[0] : 1.f, class_weight ? class_weight[1] : 1.f,
                       class_weight ? class_weight[2] : 1.f};
  const float inv2s2 = (float)(1.0 / (2.0 * (double)sigma * (double)sigma));
  const int S = WT + 2 * R;
  const size_t lds = ((size_t)S * S + (size_t)S * MW + 2) * sizeof(uint32_t);  // 66 KiB at R = WMAX_R
  allow_lds(border_weight_kernel, lds);
  dim3 grid(cdiv(w, WT), cdiv(h, WT), n);
  EUNET_REQUIRE(grid.y <= 65535u, "border_weight_map: H too large");
  border_weight_kernel<<<grid, NT, lds, (hipStream_t)stream>>>(labels, semantic, h, w, cw[0], cw[1], cw[2], w0, inv2s2,
                                                               R, out);
  EUNET_LAUNCH_CHECK("border_weight_map");
  return EUNET_OK;
}

int eunet_separate_instances(const int64_t* labels, const int64_t* semantic, int n, int h, int w, int64_t* labels_out,
                             int64_t* semantic_out, void* stream) {
  EUNET_REQUIRE(labels && labels_out && n > 0 && h > 0 && w > 0 && (semantic != nullptr) == (semantic_out != nullptr) &&
                    labels != labels_out && (!semantic || semantic != semantic_out),
                "separate_instances: bad args (semantic and semantic_out come together; not in place)");
  const long long total = (long long)n * h * w;
  const long long b = (total + NT - 1) / NT;
  const unsigned g = (unsigned)(b < 2048 ? b : 2048);
  separate_kernel<<<g, NT, 0, (hipStream_t)stream>>>(labels, semantic, total, h, w, labels_out, semantic_out);
  EUNET_LAUNCH_CHECK("separate_instances");
  return EUNET_OK;
}

}  // extern "C"
