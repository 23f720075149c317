// Learned decoder upsample: ConvTranspose2d(C, C, kernel_size=2, stride=2) behind the producing block's
// BN+ReLU, on the matrix cores (bf16: mfma_f32_16x16x32_bf16, fp32: mfma_f32_16x16x4f32).
//
//   d  = relu(fmaf(y, scale, shift))                       (rounded to the compute dtype)
//   up[n, 2i+a, 2j+b, co] = bias[co] + sum_ci d[n,i,j,ci] W[ci,co,a,b]          a, b in {0, 1}
//
// With q = 2a + b all three passes are one dense contraction, run by one tiled kernel (upconv_kernel):
//   forward   out[m][q C + co] = sum_ci  d[m][ci]  Wf[q C + co][ci]      rows = low-res pixels, K = C
//   dgrad     gd[m][ci]        = sum_k   g4[m][k]  Wd[ci][k]             k = q C + co, K = 4C
//   wgrad     dW[ci][q C + co] = sum_m   d[m][ci]  g4[m][q C + co]       K = pixels, split over pixel tiles
// where g4[m][q C + co] = g[n, 2i+a, 2j+b, co] gathers the four output pixels of input pixel m, and Wf / Wd
// are the two packed (K-contiguous) images of the torch weight [ci][co][2][2] (upconv_pack_kernel).
//
// Tiling: a block of 256 threads (4 waves as 2 x 2, 64 x 64 outputs each = 4 x 4 MFMA tiles) owns a
// UT x UT = 128 x 128 output tile and walks K in stages of 128 bytes per row.  A stage's operands are
// fetched global -> registers (16 bytes per lane, zero beyond the ragged edges) while the previous stage is
// multiplied out of LDS: the register set is the second buffer.  The forward and the data gradient keep both
// operands K-contiguous in LDS ([row][128 B + 16 B pad]; fragments are 16-byte reads, conflict-free); the
// weight gradient contracts over pixels, so its stages stay in memory order ([pixel][128 channels + pad]) and
// the fragments are gathered element-wise.  Results leave through a per-wave LDS transpose so that every lane
// stores 16 bytes of one output pixel's contiguous channels.
#include <type_traits>

#include "common.h"

EUNET_DEBUG_UNIT(upconv)

namespace {

constexpr int UT = 128;              // output tile edge (the forward's and the data gradient's pixel tile)
constexpr int NT = 256;              // threads per block
constexpr int ROWB = 144;            // forward / dgrad LDS row: 128 B of K + 16 B pad
constexpr int OPB = UT * ROWB;       // bytes of one operand stage (>= the weight gradient's stage images)
constexpr int EST = 68;              // epilogue staging row (floats): 64 + 4 pad, 16-byte aligned rows
constexpr int UNITS = 4;             // 16-byte units per thread, operand and stage (1024 / NT)
constexpr int WG_BLOCKS = 512;       // weight-gradient blocks per launch (two per CU, as conv3x3's)

enum { M_FWD = 0, M_DGRAD = 1, M_WGRAD = 2 };

struct UpArgs {
  const void* y;    // low-res pre-BN activation (fwd, wgrad)
  long long yct;
  int yco;
  const float* sc;
  const float* sh;
  const void* wp;   // packed weights: Wf (fwd) or Wd (dgrad)
  const float* bias;
  void* hi;         // high-res view: out (fwd) or g (dgrad, wgrad)
  long long hct;
  int hco;
  void* lo;         // dgrad output
  long long lct;
  int lco;
  float* dwp;       // wgrad partials [nsplit][C][4C]
  float* dbp;       // [nsplit][4][C]
  int h, w, C, M;   // low-res rows / cols, channels, pixels N h w
  int mtiles, ntiles, ktiles, per_split, nsplit;
};

// first (a = b = 0) high-res pixel index of low-res pixel m
__device__ __forceinline__ long long hi_pix00(const UpArgs& a, int m) {
  const int hw = a.h * a.w;
  const int n = m / hw, r = m - n * hw;
  const int i = r / a.w, j = r - i * a.w;
  return ((long long)n * (2 * a.h) + 2 * i) * (2ll * a.w) + 2 * j;
}
__device__ __forceinline__ long long hi_pix(const UpArgs& a, long long p00, int q) {
  const long long p = p00 + (long long)(q >> 1) * (2ll * a.w) + (q & 1);
  EUNET_DASSERT(p >= 0 && p < 4ll * a.M);
  return p;
}

// v or zeros, as a mask (a select between two 16-byte vectors was lowered through scratch memory)
__device__ __forceinline__ uint4 keep_if(uint4 v, bool ok) {
  const uint32_t m = ok ? 0xFFFFFFFFu : 0u;
  return make_uint4(v.x & m, v.y & m, v.z & m, v.w & m);
}

template <typename T>
__device__ __forceinline__ uint4 bnrelu16(uint4 raw, const float* sc, const float* sh) {
  float f[Vec16<T>::N];
  Vec16<T>::unpack(raw, f);
#pragma unroll
  for (int e = 0; e < Vec16<T>::N; ++e) {
    const float v = fmaf(f[e], sc[e], sh[e]);
    f[e] = v > 0.f ? v : 0.f;
  }
  return Vec16<T>::pack(f);
}

template <typename T, int MODE>
__global__ __launch_bounds__(NT) void upconv_kernel(const UpArgs a) {
  constexpr int E = Vec16<T>::N;             // elements per 16 bytes
  constexpr int BK = 8 * E;                  // K elements per stage (channels; wgrad: pixels)
  constexpr int CH = UT / E;                 // wgrad: 16-byte units per staged pixel
  constexpr int WPAD = sizeof(T) == 2 ? 8 : 64;
  constexpr int RSB = UT * (int)sizeof(T) + WPAD;  // wgrad: bytes per staged pixel (bank offset 16 between fragment rows)
  static_assert(BK * RSB <= OPB, "wgrad stage image");
  static_assert(4 * 16 * EST * 4 <= 2 * OPB, "epilogue staging");
  __shared__ __attribute__((aligned(16))) unsigned char lds[2 * OPB];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int wm = wv >> 1, wn = wv & 1;
  const int fr = lane & 15, fq = lane >> 4;
  int bid = blockIdx.x;
  const int nt = bid % a.ntiles;
  bid /= a.ntiles;
  const int mt = bid % a.mtiles;
  const int split = bid / a.mtiles;
  EUNET_DASSERT(split < a.nsplit);
  const int m0 = mt * UT, n0 = nt * UT;
  const int C = a.C;
  const long long K = MODE == M_FWD ? C : MODE == M_DGRAD ? 4ll * C : (long long)a.M;
  const int kt0 = split * a.per_split;
  const int kt1 = min(kt0 + a.per_split, a.ktiles);
  const T* yp = (const T*)a.y;
  const T* hp = (const T*)a.hi;
  const T* wp = (const T*)a.wp;

  // rows of this thread's staging units are fixed over K in the forward / data gradient
  long long p00[UNITS];
  if constexpr (MODE == M_DGRAD) {
#pragma unroll
    for (int i = 0; i < UNITS; ++i) {
      const int m = m0 + ((tid + i * NT) >> 3);
      p00[i] = m < a.M ? hi_pix00(a, m) : 0;
    }
  }

  uint4 ra[UNITS], rb[UNITS];
  const uint4 zero4 = make_uint4(0u, 0u, 0u, 0u);

  auto load_stage = [&](int kt) {
#pragma unroll
    for (int i = 0; i < UNITS; ++i) {
      const int u = tid + i * NT;
      // every load is issued (no branch around it: the loads of a stage stay in flight together) from an
      // index clamped into the tensor; a unit beyond a ragged edge is then replaced by zeros
      if constexpr (MODE == M_WGRAD) {
        const int rc = u % CH, kp = u / CH;
        const long long m = (long long)kt * BK + kp;  // pixel
        const int c = m0 + rc * E, n = n0 + rc * E;
        const bool okm = m < K, oka = okm && c < C;
        const int ms = okm ? (int)m : 0, cs = c < C ? c : 0;
        const int q = n / C, co = n - q * C;
        EUNET_DASSERT(q < 4);
        const uint4 va = *(const uint4*)(yp + (long long)ms * a.yct + a.yco + cs);
        const uint4 vb = *(const uint4*)(hp + hi_pix(a, hi_pix00(a, ms), q) * a.hct + a.hco + co);
        ra[i] = keep_if(va, oka);
        rb[i] = keep_if(vb, okm);
      } else {
        const int r = u >> 3, ku = u & 7;
        const long long k = (long long)kt * BK + ku * E;
        const int m = m0 + r, n = n0 + r;
        const bool okk = k < K;
        const long long ks = okk ? k : 0;
        const int ms = m < a.M ? m : 0;
        if constexpr (MODE == M_FWD) {
          const uint4 va = *(const uint4*)(yp + (long long)ms * a.yct + a.yco + ks);
          const uint4 vb = *(const uint4*)(wp + (long long)n * C + ks);  // n < 4C: 4C is a multiple of UT
          EUNET_DASSERT(n < 4 * C);
          ra[i] = keep_if(va, okk && m < a.M);
          rb[i] = keep_if(vb, okk);
        } else {
          const int q = (int)(ks / C), co = (int)(ks - (long long)q * C);
          EUNET_DASSERT(q < 4);
          const int ns = n < C ? n : 0;
          const uint4 va = *(const uint4*)(hp + hi_pix(a, p00[i], q) * a.hct + a.hco + co);
          const uint4 vb = *(const uint4*)(wp + (long long)ns * (4ll * C) + ks);
          ra[i] = keep_if(va, okk && m < a.M);
          rb[i] = keep_if(vb, okk && n < C);
        }
      }
    }
  };

  auto write_stage = [&](int kt) {
#pragma unroll
    for (int i = 0; i < UNITS; ++i) {
      const int u = tid + i * NT;
      if constexpr (MODE == M_WGRAD) {
        const int rc = u % CH, kp = u / CH;
        const long long m = (long long)kt * BK + kp;
        const int c = m0 + rc * E;
        const int cs = c < C ? c : 0;
        const uint4 vt = bnrelu16<T>(ra[i], a.sc + cs, a.sh + cs);
        const uint4 va = keep_if(vt, m < K && c < C);  // relu(shift) of a padding zero is not zero
        const int off = kp * RSB + rc * 16;
        EUNET_DASSERT(off + 16 <= OPB);
        *(uint2*)(lds + off) = make_uint2(va.x, va.y);
        *(uint2*)(lds + off + 8) = make_uint2(va.z, va.w);
        *(uint2*)(lds + OPB + off) = make_uint2(rb[i].x, rb[i].y);
        *(uint2*)(lds + OPB + off + 8) = make_uint2(rb[i].z, rb[i].w);
      } else {
        const int r = u >> 3, ku = u & 7;
        const long long k = (long long)kt * BK + ku * E;
        uint4 va = ra[i];
        if constexpr (MODE == M_FWD) {
          const long long ks = k < K ? k : 0;
          const uint4 vt = bnrelu16<T>(va, a.sc + ks, a.sh + ks);
          va = keep_if(vt, m0 + r < a.M && k < K);  // relu(shift) of a padding zero is not zero
        }
        const int off = r * ROWB + ku * 16;
        EUNET_DASSERT(off + 16 <= OPB);
        *(uint4*)(lds + off) = va;
        *(uint4*)(lds + OPB + off) = rb[i];
      }
    }
  };

  f32x4 acc[4][4];
#pragma unroll
  for (int mi = 0; mi < 4; ++mi)
#pragma unroll
    for (int ni = 0; ni < 4; ++ni) acc[mi][ni] = (f32x4){0.f, 0.f, 0.f, 0.f};
  float dbacc = 0.f;

  auto compute = [&]() {
    if constexpr (MODE == M_WGRAD) {
      const int arow = wm * 64 + fr, brow = wn * 64 + fr;
      if constexpr (sizeof(T) == 2) {
#pragma unroll
        for (int ks = 0; ks < BK / 32; ++ks) {
          s16x8 af[4], bfr[4];
#pragma unroll
          for (int j = 0; j < 8; ++j) {
            const int po = (ks * 32 + fq * 8 + j) * RSB;
#pragma unroll
            for (int t = 0; t < 4; ++t) {
              af[t][j] = *(const short*)(lds + po + (arow + t * 16) * 2);
              bfr[t][j] = *(const short*)(lds + OPB + po + (brow + t * 16) * 2);
            }
          }
#pragma unroll
          for (int mi = 0; mi < 4; ++mi)
#pragma unroll
            for (int ni = 0; ni < 4; ++ni)
              acc[mi][ni] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, af[mi]),
                                                                    __builtin_bit_cast(bf16x8, bfr[ni]), acc[mi][ni], 0, 0, 0);
        }
      } else {
#pragma unroll
        for (int ks = 0; ks < BK / 4; ++ks) {
          const int po = (ks * 4 + fq) * RSB;
          float af[4], bfr[4];
#pragma unroll
          for (int t = 0; t < 4; ++t) {
            af[t] = *(const float*)(lds + po + (arow + t * 16) * 4);
            bfr[t] = *(const float*)(lds + OPB + po + (brow + t * 16) * 4);
          }
#pragma unroll
          for (int mi = 0; mi < 4; ++mi)
#pragma unroll
            for (int ni = 0; ni < 4; ++ni)
              acc[mi][ni] = __builtin_amdgcn_mfma_f32_16x16x4f32(af[mi], bfr[ni], acc[mi][ni], 0, 0, 0);
        }
      }
    } else {
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) {
        uint4 af[4], bfr[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) {
          af[t] = *(const uint4*)(lds + (wm * 64 + t * 16 + fr) * ROWB + ks * 64 + fq * 16);
          bfr[t] = *(const uint4*)(lds + OPB + (wn * 64 + t * 16 + fr) * ROWB + ks * 64 + fq * 16);
        }
#pragma unroll
        for (int mi = 0; mi < 4; ++mi)
#pragma unroll
          for (int ni = 0; ni < 4; ++ni) {
            if constexpr (sizeof(T) == 2) {
              acc[mi][ni] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, af[mi]),
                                                                    __builtin_bit_cast(bf16x8, bfr[ni]), acc[mi][ni], 0, 0, 0);
            } else {
              // one lane holds k = 4 fq + i of both operands at step i: the same k permutation on both sides
              acc[mi][ni] = __builtin_amdgcn_mfma_f32_16x16x4f32(__uint_as_float(af[mi].x), __uint_as_float(bfr[ni].x), acc[mi][ni], 0, 0, 0);
              acc[mi][ni] = __builtin_amdgcn_mfma_f32_16x16x4f32(__uint_as_float(af[mi].y), __uint_as_float(bfr[ni].y), acc[mi][ni], 0, 0, 0);
              acc[mi][ni] = __builtin_amdgcn_mfma_f32_16x16x4f32(__uint_as_float(af[mi].z), __uint_as_float(bfr[ni].z), acc[mi][ni], 0, 0, 0);
              acc[mi][ni] = __builtin_amdgcn_mfma_f32_16x16x4f32(__uint_as_float(af[mi].w), __uint_as_float(bfr[ni].w), acc[mi][ni], 0, 0, 0);
            }
          }
      }
    }
  };

  if (kt0 < kt1) load_stage(kt0);
  for (int kt = kt0; kt < kt1; ++kt) {
    write_stage(kt);
    __syncthreads();
    if (kt + 1 < kt1) load_stage(kt + 1);
    if constexpr (MODE == M_WGRAD) {
      // bias gradient: the row-tile-0 blocks also sum their g columns over the stage's pixels (zero beyond M)
      if (mt == 0 && a.dbp != nullptr && tid < UT) {
#pragma unroll 8
        for (int kp = 0; kp < BK; ++kp) dbacc += Elem<T>::ld((const T*)(lds + OPB + kp * RSB) + tid);
      }
    }
    compute();
    __syncthreads();
  }

  // ---- epilogue: 16 rows x 64 columns per wave and pass through LDS, then 16-byte stores
  typedef typename std::conditional<MODE == M_WGRAD, float, T>::type OutT;
  constexpr int OE = 16 / (int)sizeof(OutT);  // output elements per piece
  constexpr int PPR = 64 / OE;                // pieces per row
  float* st = (float*)lds + wv * (16 * EST);
#pragma unroll
  for (int mi = 0; mi < 4; ++mi) {
#pragma unroll
    for (int ni = 0; ni < 4; ++ni)
#pragma unroll
      for (int r = 0; r < 4; ++r) st[(fq * 4 + r) * EST + ni * 16 + fr] = acc[mi][ni][r];
    __syncthreads();
#pragma unroll
    for (int pi = 0; pi < 16 * PPR / 64; ++pi) {
      const int p = lane + pi * 64;
      const int prow = p / PPR, pc = (p % PPR) * OE;
      const int grow = m0 + wm * 64 + mi * 16 + prow;
      const int gcol = n0 + wn * 64 + pc;
      float v[OE];
#pragma unroll
      for (int e = 0; e < OE; e += 4) {
        const float4 t = *(const float4*)(st + prow * EST + pc + e);
        v[e] = t.x; v[e + 1] = t.y; v[e + 2] = t.z; v[e + 3] = t.w;
      }
      if constexpr (MODE == M_FWD) {
        if (grow < a.M) {
          const int q = gcol / C, co = gcol - q * C;
          EUNET_DASSERT(q < 4 && co + OE <= C);
#pragma unroll
          for (int e = 0; e < OE; ++e) v[e] += a.bias[co + e];
          const long long P = hi_pix(a, hi_pix00(a, grow), q);
          *(uint4*)((T*)a.hi + P * a.hct + a.hco + co) = Vec16<T>::pack(v);
        }
      } else if constexpr (MODE == M_DGRAD) {
        if (grow < a.M && gcol < C) {
          EUNET_DASSERT(gcol + OE <= C);
          *(uint4*)((T*)a.lo + (long long)grow * a.lct + a.lco + gcol) = Vec16<T>::pack(v);
        }
      } else {
        if (grow < C) {
          EUNET_DASSERT(gcol + OE <= 4 * C);
          *(float4*)(a.dwp + ((long long)split * C + grow) * (4ll * C) + gcol) = make_float4(v[0], v[1], v[2], v[3]);
        }
      }
    }
    __syncthreads();
  }
  if constexpr (MODE == M_WGRAD) {
    if (mt == 0 && a.dbp != nullptr && tid < UT) {
      const int n = n0 + tid;
      const int q = n / C, co = n - q * C;
      EUNET_DASSERT(q < 4);
      a.dbp[((long long)split * 4 + q) * C + co] = dbacc;
    }
  }
}

// torch [ci][co][2][2] fp32 -> Wf [q C + co][ci] and, behind it, Wd [ci][q C + co], in the compute dtype
template <typename T>
__global__ __launch_bounds__(256) void upconv_pack_kernel(const float* w, int C, T* wp) {
  const long long total = 4ll * C * C;
  const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= total) return;
  const int k = (int)(e % (4ll * C));  // q C + co
  const int ci = (int)(e / (4ll * C));
  const int q = k / C, co = k - q * C;
  const float v = w[((long long)ci * C + co) * 4 + q];
  Elem<T>::st(wp + (long long)k * C + ci, v);
  Elem<T>::st(wp + total + e, v);
}

// the checks every pass shares: lo = the low-res side (y or gd), hi = the 2x side (out or g)
int up_check(const char* what, const eunet_act* lo, const eunet_act* hi) {
  EUNET_REQUIRE(act_ok(lo) && act_ok(hi), "%s: bad tensors", what);
  EUNET_REQUIRE(same_dtype(lo, hi), "%s: dtype mismatch", what);
  EUNET_REQUIRE(lo->c == hi->c, "%s: the layer keeps its channel count (%d vs %d)", what, lo->c, hi->c);
  EUNET_REQUIRE(lo->c % 32 == 0, "%s: channels must be a multiple of 32 (got %d)", what, lo->c);
  EUNET_REQUIRE(is_2x(hi, lo), "%s: the output is 2h x 2w of the input", what);
  EUNET_REQUIRE(vec_ok(lo) && vec_ok(hi), "%s: channel strides/offsets must be multiples of %d", what,
                elems16(lo->dtype));
  EUNET_REQUIRE(((uintptr_t)lo->ptr & 15) == 0 && ((uintptr_t)hi->ptr & 15) == 0, "%s: tensors must be 16-byte aligned", what);
  EUNET_REQUIRE((long long)lo->n * lo->h * lo->w < (1ll << 31) - UT, "%s: too many pixels", what);
  return EUNET_OK;
}

template <int MODE>
int up_launch(const UpArgs& a, int dtype, long long blocks, const char* what, void* stream) {
  EUNET_REQUIRE(blocks > 0 && blocks < (1ll << 31), "%s: grid too large", what);
  by_dtype(dtype, [&](auto t) {
    upconv_kernel<decltype(t), MODE><<<(unsigned)blocks, NT, 0, (hipStream_t)stream>>>(a);
  });
  return eunet::check_launch(what);
}

UpArgs up_args(const eunet_act* lo, const eunet_act* hi) {
  UpArgs a;
  memset(&a, 0, sizeof(a));
  a.h = lo->h; a.w = lo->w; a.C = lo->c; a.M = lo->n * lo->h * lo->w;
  a.hi = hi->ptr; a.hct = hi->ctot; a.hco = hi->coff;
  a.nsplit = 1;
  return a;
}

int stage_k(int dtype) { return dtype == EUNET_BF16 ? 64 : 32; }  // BK of upconv_kernel

}  // namespace

extern "C" {

int eunet_upconv2x2_packed_bytes(int c, int dtype, size_t* bytes) {
  EUNET_REQUIRE(bytes && c > 0 && dtype_ok(dtype), "upconv2x2_packed_bytes: bad args");
  *bytes = (size_t)8 * c * c * (dtype == EUNET_BF16 ? 2 : 4);
  return EUNET_OK;
}

int eunet_upconv2x2_pack(const float* w, int c, void* wp, int dtype, void* stream) {
  EUNET_REQUIRE(w && wp && c > 0 && dtype_ok(dtype), "upconv2x2_pack: bad args");
  EUNET_REQUIRE(c % 32 == 0, "upconv2x2_pack: channels must be a multiple of 32 (got %d)", c);
  EUNET_REQUIRE(((uintptr_t)wp & 15) == 0, "upconv2x2_pack: packed operand not 16-byte aligned");
  const long long total = 4ll * c * c;
  const unsigned grid = (unsigned)((total + 255) / 256);
  by_dtype(dtype, [&](auto t) {
    using T = decltype(t);
    upconv_pack_kernel<T><<<grid, 256, 0, (hipStream_t)stream>>>(w, c, (T*)wp);
  });
  EUNET_LAUNCH_CHECK("upconv2x2_pack");
  return EUNET_OK;
}

int eunet_bnrelu_upconv2x2_fwd(const eunet_act* y, const float* scale, const float* shift, const void* wp,
                               const float* bias, const eunet_act* out, void* stream) {
  const int rc = up_check("bnrelu_upconv2x2_fwd", y, out);
  if (rc) return rc;
  EUNET_REQUIRE(scale && shift && wp && bias, "bnrelu_upconv2x2_fwd: null scale / shift / weights / bias");
  EUNET_REQUIRE(((uintptr_t)wp & 15) == 0, "bnrelu_upconv2x2_fwd: packed operand not 16-byte aligned");
  UpArgs a = up_args(y, out);
  a.y = y->ptr; a.yct = y->ctot; a.yco = y->coff;
  a.sc = scale; a.sh = shift; a.wp = wp; a.bias = bias;
  a.mtiles = cdiv(a.M, UT); a.ntiles = 4 * a.C / UT;
  a.ktiles = cdiv(a.C, stage_k(y->dtype)); a.per_split = a.ktiles;
  return up_launch<M_FWD>(a, y->dtype, (long long)a.mtiles * a.ntiles, "bnrelu_upconv2x2_fwd", stream);
}

int eunet_upconv2x2_dgrad(const eunet_act* g, const void* wp, const eunet_act* gd, void* stream) {
  const int rc = up_check("upconv2x2_dgrad", gd, g);
  if (rc) return rc;
  EUNET_REQUIRE(wp && ((uintptr_t)wp & 15) == 0, "upconv2x2_dgrad: packed operand null or not 16-byte aligned");
  UpArgs a = up_args(gd, g);
  a.lo = gd->ptr; a.lct = gd->ctot; a.lco = gd->coff;
  const size_t esz = g->dtype == EUNET_BF16 ? 2 : 4;
  a.wp = (const char*)wp + (size_t)4 * a.C * a.C * esz;  // Wd follows Wf
  a.mtiles = cdiv(a.M, UT); a.ntiles = cdiv(a.C, UT);
  a.ktiles = cdiv(4 * a.C, stage_k(g->dtype)); a.per_split = a.ktiles;
  return up_launch<M_DGRAD>(a, g->dtype, (long long)a.mtiles * a.ntiles, "upconv2x2_dgrad", stream);
}

int eunet_upconv2x2_wgrad_splits(const eunet_act* y, int dtype, int* nsplit) {
  EUNET_REQUIRE(act_ok(y) && nsplit && dtype_ok(dtype), "upconv2x2_wgrad_splits: bad args");
  const long long M = (long long)y->n * y->h * y->w;
  const long long ktiles = (M + stage_k(dtype) - 1) / stage_k(dtype);
  const int blocks = cdiv(y->c, UT) * cdiv(4 * y->c, UT);
  long long s = cdiv(WG_BLOCKS, blocks);
  s = s > ktiles ? ktiles : s;
  const long long per = 4ll * y->c * y->c * 4;  // keep the partials <= 256 MiB
  while (s > 1 && per * s > (256ll << 20)) --s;
  const long long per_split = (ktiles + s - 1) / s;
  *nsplit = (int)((ktiles + per_split - 1) / per_split);
  return EUNET_OK;
}

int eunet_upconv2x2_wgrad(const eunet_act* y, const float* scale, const float* shift, const eunet_act* g,
                          float* dw_part, float* db_part, int nsplit, void* stream) {
  const int rc = up_check("upconv2x2_wgrad", y, g);
  if (rc) return rc;
  EUNET_REQUIRE(scale && shift && dw_part && nsplit > 0, "upconv2x2_wgrad: bad args");
  EUNET_REQUIRE(((uintptr_t)dw_part & 15) == 0, "upconv2x2_wgrad: partials not 16-byte aligned");
  UpArgs a = up_args(y, g);
  a.y = y->ptr; a.yct = y->ctot; a.yco = y->coff;
  a.sc = scale; a.sh = shift; a.dwp = dw_part; a.dbp = db_part;
  a.mtiles = cdiv(a.C, UT); a.ntiles = 4 * a.C / UT;
  a.ktiles = cdiv(a.M, stage_k(y->dtype));
  a.per_split = cdiv(a.ktiles, nsplit);
  a.nsplit = nsplit;
  EUNET_REQUIRE(cdiv(a.ktiles, a.per_split) == nsplit, "upconv2x2_wgrad: nsplit not from upconv2x2_wgrad_splits");
  return up_launch<M_WGRAD>(a, y->dtype, (long long)nsplit * a.mtiles * a.ntiles, "upconv2x2_wgrad", stream);
}

}  // extern "C"
