// Kernels of ControlNet's HED annotator (modules/annotator/hed/__init__.py), fp32 class: what stands between the VGG trunk's 3 x 3 convs,
// and the detector's tail.
//
// crg_relu_pool_proj: one pass over a conv's fp32 output x [N][H][W][C].  r = x > 0 ? x : 0, and out of the same registers any of
//   the half-type planes of r (the next conv of the block), the planes of maxpool2x2(r) (the next block's first conv) and the block's
//   1-channel 1 x 1 `projection` conv of r.  A lane owns 8 consecutive channels of one 2 x 2 window (of a partial one on the last row /
//   column of an odd image: those pixels have planes and a projection but no pooled value): eight 16-byte loads in flight per lane, one
//   16-byte store per plane and pixel.  L = C / 8 lanes share a window; a block of 256 threads takes 256 / L windows, consecutive along
//   the image row, so a block reads whole runs of a row pair.  The projection: per lane acc = fma(w[c], r[c], acc) over its 8 channels in
//   channel order, then over the L lanes of the pixel
//     - L a power of two up to 64: an xor butterfly (offsets 1, 2, .. L / 2) inside the wave - the groups do not straddle waves;
//     - any other L (C = 72: 9 lanes): the partials go through LDS and one lane sums them in lane order.
//   Either order is a function of C alone: nothing depends on N, H, W, the grid or the batch-invariant mode.  No atomics.
//
// crg_hed_fuse: HEDdetector.__call__'s tail (:73-77) in one launch: up to 8 side maps [N][h_i][w_i] resized to [H][W] with the bilinear
//   tables of postprocess.hed_tables (index, fraction per output column and row, built in double on the host), summed in map order, divided
//   by the count, the sigmoid in double, bytes by truncation.  The definition is postprocess.hed_fuse_host and the values are equal, so
//   NOTHING in this file may contract a multiply and an add into one rounding where the definition has two: the fuse kernel is compiled
//   with contraction off, the projection uses explicit fmaf.
#include <math.h>

#include "crg_common.h"

#pragma clang fp contract(off)  // file scope: every function below

namespace {
constexpr int RP_THREADS = 256;
constexpr int RP_MAX_C = 2048;  // 256 lanes of 8 channels: one window per block

struct RpP {
  const float* x;
  bf16* hi; bf16* lo;    // [N][H][W][C] or null
  bf16* phi; bf16* plo;  // [N][H/2][W/2][C] or null
  const float* w; const float* bias; float* proj;  // [C], [1] or null, [N][H][W] or null
  int H, W, C, L, G, Hc, Wc, shuffle;
  long units;  // N * Hc * Wc windows
};

__device__ __forceinline__ void rp_split_store(const float (&f)[8], bf16* hi, bf16* lo, long off) {
  bf16x8 h8, l8;
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const bf16 h = (bf16)f[e];
    h8[e] = h;
    l8[e] = (bf16)(f[e] - (float)h);
  }
  *reinterpret_cast<bf16x8*>(hi + off) = h8;
  *reinterpret_cast<bf16x8*>(lo + off) = l8;
}

__global__ __launch_bounds__(RP_THREADS) void relu_pool_proj_kernel(const RpP p) {
  __shared__ float part[4][RP_THREADS];
  const int t = threadIdx.x;
  const int g = t / p.L, j = t - g * p.L;  // window of the block, lane of the window
  const long unit = (long)blockIdx.x * p.G + g;
  const bool live = g < p.G && unit < p.units;
  float acc[4] = {0.f, 0.f, 0.f, 0.f};
  int n = 0, wy = 0, wx = 0;
  if (live) {
    const long per = (long)p.Hc * p.Wc;
    n = (int)(unit / per);
    const int r = (int)(unit - (long)n * per);
    wy = r / p.Wc;
    wx = r - wy * p.Wc;
    const int c0 = j * 8;
    const int y0 = 2 * wy, x0 = 2 * wx;
    const bool ok[4] = {true, x0 + 1 < p.W, y0 + 1 < p.H, x0 + 1 < p.W && y0 + 1 < p.H};
    f32x4 a[4], b[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {  // all loads first: eight in flight
      a[q] = f32x4{0.f, 0.f, 0.f, 0.f};
      b[q] = a[q];
      if (ok[q]) {
        const float* src = p.x + (((long)n * p.H + y0 + (q >> 1)) * p.W + x0 + (q & 1)) * p.C + c0;
        a[q] = *reinterpret_cast<const f32x4*>(src);
        b[q] = *reinterpret_cast<const f32x4*>(src + 4);
      }
    }
    float wv[8];
    if (p.proj) {
      const f32x4 w0 = *reinterpret_cast<const f32x4*>(p.w + c0), w1 = *reinterpret_cast<const f32x4*>(p.w + c0 + 4);
#pragma unroll
      for (int e = 0; e < 8; ++e) wv[e] = e < 4 ? w0[e] : w1[e - 4];
    }
    float mx[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) mx[e] = 0.f;  // r >= 0: zero is the identity of the window's max
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      if (!ok[q]) continue;
      float r8[8];
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const float v = e < 4 ? a[q][e] : b[q][e - 4];
        r8[e] = v > 0.f ? v : 0.f;
        mx[e] = r8[e] > mx[e] ? r8[e] : mx[e];
      }
      if (p.hi) rp_split_store(r8, p.hi, p.lo, (((long)n * p.H + y0 + (q >> 1)) * p.W + x0 + (q & 1)) * p.C + c0);
      if (p.proj) {
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[q] = __builtin_fmaf(wv[e], r8[e], acc[q]);
      }
    }
    if (p.phi && ok[3]) rp_split_store(mx, p.phi, p.plo, (((long)n * (p.H / 2) + wy) * (p.W / 2) + wx) * p.C + c0);
  }
  if (!p.proj) return;  // (uniform: a kernel argument)
  if (p.shuffle) {  // L a power of two <= 64, RP_THREADS % L == 0: a window's lanes are L consecutive lanes of one wave
#pragma unroll
    for (int q = 0; q < 4; ++q)
      for (int o = 1; o < p.L; o <<= 1) acc[q] = acc[q] + __shfl_xor(acc[q], o);
  } else {
#pragma unroll
    for (int q = 0; q < 4; ++q) part[q][t] = acc[q];
    __syncthreads();
    if (live && j == 0) {
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        float s = part[q][t];
        for (int i = 1; i < p.L; ++i) s = s + part[q][t + i];
        acc[q] = s;
      }
    }
  }
  if (live && j == 0) {
    const int y0 = 2 * wy, x0 = 2 * wx;
    const float bias = p.bias ? p.bias[0] : 0.f;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int y = y0 + (q >> 1), x = x0 + (q & 1);
      if (y < p.H && x < p.W) p.proj[((long)n * p.H + y) * p.W + x] = bias + acc[q];
    }
  }
}

// ---- the detector's tail --------------------------------------------------------------------------------------------------------------
constexpr int HF_MAPS = 8;
struct HfP {
  const float* map[HF_MAPS];
  int h[HF_MAPS], w[HF_MAPS];
  const int* idx; const float* frac;  // per map: [W] columns then [H] rows, map m at m * (W + H)
  unsigned char* out; float* mean;
  int n_maps, H, W;
};

// One thread per output pixel, a block 64 x 4 pixels of sample blockIdx.z.  Per map, as postprocess.hed_fuse_host: the two source rows
// interpolated horizontally, then vertically, each operation rounded to fp32; a map already at (H, W) is copied.
__global__ __launch_bounds__(256) void hed_fuse_kernel(const HfP p) {
  const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
  if (x >= p.W || y >= p.H) return;
  const int n = blockIdx.z;
  float sum = 0.f;
  for (int m = 0; m < p.n_maps; ++m) {
    const int h = p.h[m], w = p.w[m];
    const float* s = p.map[m] + (long)n * h * w;
    float v;
    if (h == p.H && w == p.W) {
      v = s[(long)y * w + x];
    } else {
      const long tb = (long)m * (p.W + p.H);
      int sx = p.idx[tb + x], sy = p.idx[tb + p.W + y];
      sx = sx < 0 ? 0 : (sx < w ? sx : w - 1);  // (a table never leaves its map; nothing outside one is addressed whatever it holds)
      sy = sy < 0 ? 0 : (sy < h ? sy : h - 1);
      const float fx = p.frac[tb + x], fy = p.frac[tb + p.W + y];
      const int sx1 = sx + 1 < w ? sx + 1 : w - 1, sy1 = sy + 1 < h ? sy + 1 : h - 1;
      const float gx = 1.0f - fx, gy = 1.0f - fy;
      const float r0 = s[(long)sy * w + sx] * gx + s[(long)sy * w + sx1] * fx;
      const float r1 = s[(long)sy1 * w + sx] * gx + s[(long)sy1 * w + sx1] * fx;
      v = r0 * gy + r1 * fy;
    }
    sum = m == 0 ? v : sum + v;
  }
  const float mean = sum / (float)p.n_maps;
  const long o = ((long)n * p.H + y) * p.W + x;
  if (p.mean) p.mean[o] = mean;
  const double e = 1.0 / (1.0 + exp(-(double)mean));
  const double q = fmin(fmax(e * 255.0, 0.0), 255.0);
  p.out[o] = (unsigned char)(int)q;
}

inline bool rp_disjoint(const void* a, size_t na, const void* b, size_t nb) {
  const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
  return !a || !b || a0 + na <= b0 || b0 + nb <= a0;
}
}  // namespace

extern "C" int crg_relu_pool_proj(crg_ctx* ctx, void* stream, const float* x, void* hi, void* lo, void* pool_hi, void* pool_lo, const float* proj_w,
                                  const float* proj_bias, float* proj, int N, int H, int W, int C) {
  if (!ctx) return -22;
  CRG_REQUIRE(ctx, x, "relu_pool_proj: null input");
  CRG_REQUIRE(ctx, (hi == nullptr) == (lo == nullptr) && (pool_hi == nullptr) == (pool_lo == nullptr), "relu_pool_proj: both planes of a pair or none");
  CRG_REQUIRE(ctx, hi || pool_hi || proj, "relu_pool_proj: nothing to write");
  CRG_REQUIRE(ctx, !proj || proj_w, "relu_pool_proj: a projection needs its weight");
  CRG_REQUIRE(ctx, N >= 1 && H >= 1 && W >= 1, "relu_pool_proj: empty problem N=%d H=%d W=%d", N, H, W);
  CRG_REQUIRE(ctx, C >= 8 && C % 8 == 0 && C <= RP_MAX_C, "relu_pool_proj: C=%d must be a multiple of 8, at most %d", C, RP_MAX_C);
  CRG_REQUIRE(ctx, !pool_hi || (H >= 2 && W >= 2), "relu_pool_proj: a %d x %d image has no 2 x 2 window", H, W);
  CRG_REQUIRE(ctx, (((uintptr_t)x | (uintptr_t)hi | (uintptr_t)lo | (uintptr_t)pool_hi | (uintptr_t)pool_lo | (uintptr_t)proj_w) & 15) == 0 &&
                       (((uintptr_t)proj | (uintptr_t)proj_bias) & 3) == 0,
              "relu_pool_proj: x, the planes and the weight must be 16-byte aligned");
  const int64_t px = (int64_t)N * H * W, ppx = (int64_t)N * (H / 2) * (W / 2);
  CRG_REQUIRE(ctx, px < (1LL << 31), "relu_pool_proj: %lld pixels are beyond 2^31", (long long)px);
  {
    const size_t xb = (size_t)px * C * 4, pb = (size_t)px * C * sizeof(bf16), qb = (size_t)ppx * C * sizeof(bf16), jb = (size_t)px * 4;
    const void* outs[5] = {hi, lo, pool_hi, pool_lo, proj};
    const size_t nb[5] = {pb, pb, qb, qb, jb};
    for (int i = 0; i < 5; ++i) {
      CRG_REQUIRE(ctx, rp_disjoint(outs[i], nb[i], x, xb) && rp_disjoint(outs[i], nb[i], proj_w, (size_t)C * 4), "relu_pool_proj: an output overlaps an input");
      for (int k = i + 1; k < 5; ++k) CRG_REQUIRE(ctx, rp_disjoint(outs[i], nb[i], outs[k], nb[k]), "relu_pool_proj: two outputs overlap");
    }
  }
  RpP p = {};
  p.x = x; p.hi = (bf16*)hi; p.lo = (bf16*)lo; p.phi = (bf16*)pool_hi; p.plo = (bf16*)pool_lo;
  p.w = proj_w; p.bias = proj_bias; p.proj = proj;
  p.H = H; p.W = W; p.C = C; p.L = C / 8; p.G = RP_THREADS / p.L;
  p.Hc = (H + 1) / 2; p.Wc = (W + 1) / 2;
  p.units = (long)N * p.Hc * p.Wc;
  p.shuffle = (p.L <= 64 && (p.L & (p.L - 1)) == 0) ? 1 : 0;
  const long blocks = (p.units + p.G - 1) / p.G;
  CRG_REQUIRE(ctx, blocks <= 0x7fffffffL, "relu_pool_proj: %ld blocks exceed the grid", blocks);
  hipStream_t st = (hipStream_t)stream;
  const double elems = (double)px * C;
  crg_prof_scope ps(ctx, st, CRG_K_ELEMENTWISE, elems * (2.0 + (proj ? 2.0 : 0.0) + (hi ? 2.0 : 0.0)),
                    elems * (4.0 + (hi ? 4.0 : 0.0)) + (pool_hi ? 4.0 * ppx * C : 0.0) + (proj ? 4.0 * px : 0.0));
  hipLaunchKernelGGL(relu_pool_proj_kernel, dim3((unsigned)blocks), dim3(RP_THREADS), 0, st, p);
  CRG_CHECK_LAUNCH(ctx, "relu_pool_proj");
  return 0;
}

extern "C" int crg_hed_fuse(crg_ctx* ctx, void* stream, int n_maps, const void* const* maps, const int* map_h, const int* map_w, const int* tab_idx,
                            const float* tab_frac, void* out, float* mean, int N, int H, int W) {
  if (!ctx) return -22;
  CRG_REQUIRE(ctx, n_maps >= 1 && n_maps <= HF_MAPS, "hed_fuse: %d side maps (1..%d)", n_maps, HF_MAPS);
  CRG_REQUIRE(ctx, maps && map_h && map_w && tab_idx && tab_frac && out, "hed_fuse: null maps, sizes, tables or output");
  CRG_REQUIRE(ctx, N >= 1 && H >= 1 && W >= 1 && N <= 65535 && (H + 3) / 4 <= 65535, "hed_fuse: empty or oversized output (N=%d H=%d W=%d)", N, H, W);
  CRG_REQUIRE(ctx, (int64_t)N * H * W < (1LL << 31), "hed_fuse: the output is beyond 2^31 pixels");
  const size_t ob = (size_t)N * H * W, tb = (size_t)n_maps * ((size_t)W + H) * 4;
  HfP p = {};
  for (int m = 0; m < n_maps; ++m) {
    CRG_REQUIRE(ctx, maps[m] && map_h[m] >= 1 && map_w[m] >= 1, "hed_fuse: side map %d is null or empty (%d x %d)", m, map_h[m], map_w[m]);
    CRG_REQUIRE(ctx, ((uintptr_t)maps[m] & 3) == 0 && (int64_t)N * map_h[m] * map_w[m] < (1LL << 31), "hed_fuse: side map %d is misaligned or too large", m);
    const size_t mb = (size_t)N * map_h[m] * map_w[m] * 4;
    CRG_REQUIRE(ctx, rp_disjoint(out, ob, maps[m], mb) && rp_disjoint(mean, ob * 4, maps[m], mb), "hed_fuse: an output overlaps side map %d", m);
    p.map[m] = (const float*)maps[m];
    p.h[m] = map_h[m];
    p.w[m] = map_w[m];
  }
  CRG_REQUIRE(ctx, rp_disjoint(out, ob, mean, ob * 4) && rp_disjoint(out, ob, tab_idx, tb) && rp_disjoint(out, ob, tab_frac, tb) &&
                       rp_disjoint(mean, ob * 4, tab_idx, tb) && rp_disjoint(mean, ob * 4, tab_frac, tb),
              "hed_fuse: the outputs overlap each other or the tables");
  CRG_REQUIRE(ctx, (((uintptr_t)tab_idx | (uintptr_t)tab_frac | (uintptr_t)mean) & 3) == 0, "hed_fuse: tables and mean field must be 4-byte aligned");
  p.idx = tab_idx; p.frac = tab_frac; p.out = (unsigned char*)out; p.mean = mean;
  p.n_maps = n_maps; p.H = H; p.W = W;
  hipStream_t st = (hipStream_t)stream;
  const double px = (double)ob;
  crg_prof_scope ps(ctx, st, CRG_K_ELEMENTWISE, px * (10.0 * n_maps + 30.0), px * (16.0 * n_maps + 1.0 + (mean ? 4.0 : 0.0)));
  hipLaunchKernelGGL(hed_fuse_kernel, dim3((W + 63) / 64, (H + 3) / 4, N), dim3(256), 0, st, p);
  CRG_CHECK_LAUNCH(ctx, "hed_fuse");
  return 0;
}
