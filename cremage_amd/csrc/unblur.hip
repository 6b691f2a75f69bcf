// Kernels of the face unblur / colorize network (modules/unblur_face/cremage_model_v6.py), fp32 class.
//
// crg_conv_transpose2d: ConvTranspose2d(kernel 4, stride 2, padding 1) as four parity GEMMs on the SOURCE grid, one launch (blockIdx.y =
//   parity).  For output parity (a, b)
//       y[2i+a][2j+b] = sum_{u,v in {0,1}}  w[:, :, 3-a-2u, 3-b-2v]^T  x[i+a-1+u][j+b-1+v]
//   so a block's A rows are the source pixels of a 32 / 128-row tile, gathered per tap (u, v) at a fixed row offset (a-1+u) W + (b-1+v)
//   of the SAME planes; a tap whose source pixel lies outside the image is staged from the context's zero page BY SELECTION - rows of
//   the next image line / sample are never addressed.  No zero-stuffed image exists, and the weight image (CRG_PACK_CONVT_UP2) holds only
//   the four taps a parity reads: nothing structurally zero is streamed or multiplied.  On a 1-row (1-column) grid the taps that no
//   pixel of the grid can reach (u != 1 - a, v != 1 - b) are not walked at all: at 1 x 1 each weight byte the output depends on is read
//   once and the others never.
//   Structure of conv_frames_x3_kernel (video_x3.hip): operands as the hi / lo 16-bit planes, LDS-DMA in 16-byte pieces into the
//   XOR-swizzled 128-byte-row image, one stage of four planes [X hi][X lo][W hi][W lo], three MFMA passes lo*hi + hi*lo + hi*hi per
//   k-step into one fp32 accumulator, the whole K of a tile summed by one block in a fixed order (no split-K).  Epilogue: bias, SiLU
//   (ConvTransposeAct), fp32 stores to the interleaved output pixel.
//
// crg_groupnorm_add_act: y = silu?(GroupNorm(x) + skip), the tail of the network's post-norm residual blocks, with the hi / lo planes
//   of y for the next fp32-class conv out of the same pass.  Launch 1 folds the statistics per (sample, group, row slice) - from x, or
//   from the producing conv's gn_stats side channel - into fp64 partials; launch 2 reads x and skip once and writes y and the planes.
#include <math.h>

#include "gemm_shared.h"

namespace {
using crg_mm::BK;
using crg_mm::gptr_t;
using crg_mm::lds_off;
using crg_mm::lptr_t;
using crg_mm::wait_vmcnt;

// the arguments of the two entry points, gathered (include/crg_hip.h has them flat)
struct crg_conv_transpose_args {
  const void* x_hi; const void* x_lo; const void* w_hi; const void* w_lo; const float* bias; void* y;
  int N, H, W, Cin, Cout, silu;
};
struct crg_gn_add_act_args {
  const void* x; const void* skip; int64_t ld_skip; const float* gamma; const float* beta; const float* gn_stats;
  void* y; int64_t ld_y; void* y_hi; void* y_lo; int64_t ld_planes; void* workspace; int64_t workspace_bytes;
  int N, HW, C, groups; float eps; int silu;
};

struct CtP {
  const bf16* x_hi; const bf16* x_lo; const bf16* w_hi; const bf16* w_lo;
  const float* bias; float* y; const bf16* zpage;
  int M, N, Cin, H, W, tiles_n, silu, cm, kchunks;
};

template <int WNT, int WMT, int NS>
constexpr int ct_lds_bytes() { return NS * 2 * (32 * WMT * 128 + 32 * WNT * 128); }
static_assert(2 * ct_lds_bytes<4, 4, 1>() <= 160 * 1024, "four planes at the 128 x 128 tile: 64 KB, two blocks per CU");
static_assert(ct_lds_bytes<1, 1, 8>() <= 160 * 1024 && ct_lds_bytes<1, 2, 6>() <= 160 * 1024, "the rings of the small grids: one block per CU");

// BM = 32 WMT source pixels x BN = 32 WNT output channels of one parity; 4 waves as 2 x 2, a wave owns 16 WMT rows x 16 WNT columns.
// NS: stages of the LDS ring.  The small grids are bound by the weight stream and have fewer blocks than the device has CUs, so what
// keeps HBM busy is the number of k-tiles each block has in flight: NS - 1 of them while it multiplies the oldest.  Every wave issues the
// same 2 (WMT + WNT) DMA instructions per stage - beyond the last k-tile they read the zero page - so the wait is a counted one.
template <int WNT, int WMT, int NS>
__global__ __launch_bounds__(256, 2) void conv_transpose_kernel(const CtP p) {
  constexpr int BM = 32 * WMT, BN = 32 * WNT;
  constexpr int XS_BYTES = BM * 128, WS_BYTES = BN * 128;  // a stage: [X hi][X lo][W hi][W lo]
  constexpr int STAGE_BYTES = 2 * (XS_BYTES + WS_BYTES), PER_STAGE = 2 * (WMT + WNT);
  static_assert((NS - 1) * PER_STAGE < 64, "vmcnt is 6 bits");
  extern __shared__ __attribute__((aligned(16))) char ct_smem[];

  const int t = threadIdx.x, lane = t & 63;
  const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
  const int wm = wave >> 1, wn = wave & 1;
  const int tile_n = blockIdx.x % p.tiles_n, tile_m = blockIdx.x / p.tiles_n;
  const int par = blockIdx.y, pa = par >> 1, pb = par & 1;
  const int m0 = tile_m * BM, n0 = tile_n * BN;
  const int HW = p.H * p.W;

  // this lane stages LDS row 8 g + lane / 8, physical chunk lane % 8 of row group g = wave + 4 q; it carries logical chunk clog
  const int rsub = lane >> 3, clog = (lane & 7) ^ rsub;
  long xoff[WMT];
  int xmask[WMT];  // bit 2 u + v: the source pixel of tap (u, v) is inside the image
#pragma unroll
  for (int q = 0; q < WMT; ++q) {
    const int m = m0 + (wave + 4 * q) * 8 + rsub;
    const int r = m % HW, i = r / p.W, j = r - i * p.W;
    int mask = 0;
#pragma unroll
    for (int tap = 0; tap < 4; ++tap) {
      const int si = i + pa - 1 + (tap >> 1), sj = j + pb - 1 + (tap & 1);
      if (m < p.M && si >= 0 && si < p.H && sj >= 0 && sj < p.W) mask |= 1 << tap;
    }
    xmask[q] = mask;
    xoff[q] = (long)m * p.Cin;
  }
  const long K = 4L * p.Cin;
  long woff[WNT];
  bool wok[WNT];
#pragma unroll
  for (int q = 0; q < WNT; ++q) {
    const int n = n0 + (wave + 4 * q) * 8 + rsub;
    wok[q] = n < p.N;
    woff[q] = ((long)par * p.N + n) * K;
  }
  // the taps some pixel of the grid reaches: both u unless H == 1 (then only u = 1 - a), both v unless W == 1
  const int nu = p.H > 1 ? 2 : 1, nv = p.W > 1 ? 2 : 1;
  const int nk = nu * nv * p.kchunks;

  auto stage = [&](int kt, int slot) {
    const int lt = kt / p.kchunks, cc = kt - lt * p.kchunks;
    const int lu = lt / nv, lv = lt - lu * nv;
    const int u = p.H > 1 ? lu : 1 - pa, v = p.W > 1 ? lv : 1 - pb;
    const int tap = 2 * u + v;
    const int c = cc * BK + clog * 8;
    const bool cok = c < p.Cin && kt < nk;  // (beyond the last k-tile: the zero page, nothing computed above is dereferenced)
    const long xrel = (long)((pa - 1 + u) * p.W + (pb - 1 + v)) * p.Cin + c;  // only added to a plane's base when the tap is inside
    const long wrel = p.cm ? (long)cc * (4 * BK) + tap * BK + clog * 8 : (long)tap * p.Cin + c;
    char* xs = ct_smem + slot * STAGE_BYTES;
    char* ws = xs + 2 * XS_BYTES;
#pragma unroll
    for (int q = 0; q < WMT; ++q) {
      const bool ok = cok && ((xmask[q] >> (tap & 3)) & 1);
      const bf16* sh = ok ? p.x_hi + xoff[q] + xrel : p.zpage;
      const bf16* sl = ok ? p.x_lo + xoff[q] + xrel : p.zpage;
      __builtin_amdgcn_global_load_lds((gptr_t)sh, (lptr_t)(xs + (wave + 4 * q) * 1024), 16, 0, 0);
      __builtin_amdgcn_global_load_lds((gptr_t)sl, (lptr_t)(xs + XS_BYTES + (wave + 4 * q) * 1024), 16, 0, 0);
    }
#pragma unroll
    for (int q = 0; q < WNT; ++q) {
      const bool ok = cok && wok[q];
      const bf16* sh = ok ? p.w_hi + woff[q] + wrel : p.zpage;
      const bf16* sl = ok ? p.w_lo + woff[q] + wrel : p.zpage;
      __builtin_amdgcn_global_load_lds((gptr_t)sh, (lptr_t)(ws + (wave + 4 * q) * 1024), 16, 0, 0);
      __builtin_amdgcn_global_load_lds((gptr_t)sl, (lptr_t)(ws + WS_BYTES + (wave + 4 * q) * 1024), 16, 0, 0);
    }
  };

  f32x4 acc[WNT][WMT];
#pragma unroll
  for (int i = 0; i < WNT; ++i)
#pragma unroll
    for (int j = 0; j < WMT; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  const int frow = lane & 15, fq = lane >> 4;

#pragma unroll
  for (int s = 0; s < NS; ++s) stage(s, s);
  int slot = 0;
  for (int kt = 0; kt < nk; ++kt) {
    const char* xs = ct_smem + slot * STAGE_BYTES;
    const char* ws = xs + 2 * XS_BYTES;
    wait_vmcnt<(NS - 1) * PER_STAGE>();  // all but the NS - 1 youngest stages of this wave have landed: k-tile kt is among them
    asm volatile("" ::: "memory");
    __builtin_amdgcn_s_barrier();  // ... for every wave
    asm volatile("" ::: "memory");
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      bf16x8 xf[WMT], xl[WMT], wf[WNT], wl[WNT];
#pragma unroll
      for (int j = 0; j < WMT; ++j) {
        const int off = lds_off(wm * (16 * WMT) + j * 16 + frow, ks * 4 + fq);
        xf[j] = *reinterpret_cast<const bf16x8*>(xs + off);
        xl[j] = *reinterpret_cast<const bf16x8*>(xs + XS_BYTES + off);
      }
#pragma unroll
      for (int i = 0; i < WNT; ++i) {
        const int off = lds_off(wn * (16 * WNT) + i * 16 + frow, ks * 4 + fq);
        wf[i] = *reinterpret_cast<const bf16x8*>(ws + off);
        wl[i] = *reinterpret_cast<const bf16x8*>(ws + WS_BYTES + off);
      }
#pragma unroll
      for (int i = 0; i < WNT; ++i)
#pragma unroll
        for (int j = 0; j < WMT; ++j) {  // the small products first, as in conv_frames_x3_kernel
          acc[i][j] = CRG_MFMA_16x16x32(wl[i], xf[j], acc[i][j]);
          acc[i][j] = CRG_MFMA_16x16x32(wf[i], xl[j], acc[i][j]);
          acc[i][j] = CRG_MFMA_16x16x32(wf[i], xf[j], acc[i][j]);
        }
    }
    asm volatile("" ::: "memory");
    __builtin_amdgcn_s_barrier();  // everybody is done reading before k-tile kt + NS overwrites the slot
    asm volatile("" ::: "memory");
    stage(kt + NS, slot);
    slot = slot + 1 == NS ? 0 : slot + 1;
  }
  wait_vmcnt<0>();  // the trailing zero-page stages

  // lane: source pixel m = .. + frow, output channels n .. n + 3 of each 16 x 16 tile (N % 4 == 0: a group of four is in or out as a whole)
#pragma unroll
  for (int j = 0; j < WMT; ++j) {
    const int m = m0 + wm * (16 * WMT) + j * 16 + frow;
    if (m >= p.M) continue;
    const int s = m / HW, r = m - s * HW, si = r / p.W, sj = r - si * p.W;
    const long orow = ((long)s * 2 * p.H + 2 * si + pa) * (2 * p.W) + 2 * sj + pb;
#pragma unroll
    for (int i = 0; i < WNT; ++i) {
      const int n = n0 + wn * (16 * WNT) + i * 16 + fq * 4;
      if (n >= p.N) continue;
      f32x4 v = acc[i][j];
      if (p.bias) v += *reinterpret_cast<const f32x4*>(p.bias + n);
      if (p.silu) {
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = v[e] / (1.0f + expf(-v[e]));
      }
      *reinterpret_cast<f32x4*>(p.y + orow * p.N + n) = v;
    }
  }
}

template <int WNT, int WMT, int NS>
int launch_conv_transpose(crg_ctx* ctx, hipStream_t st, CtP& p) {
  const void* kern = reinterpret_cast<const void*>(&conv_transpose_kernel<WNT, WMT, NS>);
  if (int rc = crg_set_dyn_lds(ctx, kern, ct_lds_bytes<WNT, WMT, NS>(), "conv_transpose2d")) return rc;
  p.tiles_n = (p.N + 32 * WNT - 1) / (32 * WNT);
  const long tiles = (long)((p.M + 32 * WMT - 1) / (32 * WMT)) * p.tiles_n;
  if (tiles > 0x7fffffffL) return crg_fail(ctx, -22, "conv_transpose2d: %ld tiles exceed the grid", tiles);
  const int lds = ct_lds_bytes<WNT, WMT, NS>();
  hipLaunchKernelGGL((conv_transpose_kernel<WNT, WMT, NS>), dim3((unsigned)tiles, 4), dim3(256), lds, st, p);
  CRG_CHECK_LAUNCH(ctx, "conv_transpose2d");
  return 0;
}

// The host-side plan.  Up to 64 source pixels (the 1 x 1 .. 8 x 8 grids of one face): 32 x 32 tiles and a ring of 8 stages; up to 512
// (16 x 16): 64 x 32 tiles and a ring of 6; beyond, one stage and two blocks per CU, 128 rows, the tile width the widest of 128 / 64 / 32
// that still gives every CU a block.
struct CtPlan { int wnt, wmt, ns; };
inline CtPlan plan_conv_transpose(long rows, int cout, int cus) {
  CtPlan pl;
  pl.wnt = 1;
  if (rows <= 64) {
    pl.wmt = 1, pl.ns = 8;
    return pl;
  }
  if (rows <= 512) {
    pl.wmt = 2, pl.ns = 6;
    return pl;
  }
  pl.wmt = 4, pl.ns = 1;
  const long tiles_m = (rows + 32 * pl.wmt - 1) / (32 * pl.wmt);
  for (int w = 4; w > 1; w >>= 1)
    if (cout >= 32 * w && 4 * tiles_m * ((cout + 32 * w - 1) / (32 * w)) >= cus) {
      pl.wnt = w;
      break;
    }
  return pl;
}

// ---- GroupNorm + residual + SiLU ---------------------------------------------------------------------------------------------------
constexpr int GA_MAX_GROUPS = 64, GA_MAX_SLICES = 64, GA_SLICE_ROWS = 1024;

// partial (sum, sum of squares) of rows [slice * rows_per, ..) of group g of sample n, in fp64: ws[((n * G + g) * S + slice) * 2 + {0, 1}]
__global__ __launch_bounds__(256) void gn_add_stats_kernel(const float* __restrict__ x, const float* __restrict__ stats, long stats_plane, double* __restrict__ ws,
                                                           int HW, int C, int G, int S, int rows_per) {
  __shared__ double red[2][4];
  const int ng = blockIdx.x, n = ng / G, g = ng - n * G, slice = blockIdx.y, cpg = C / G;
  double s = 0.0, ss = 0.0;
  if (stats) {  // the producer's partials: per 32-row block and channel, rows_per is a multiple of 32 then
    const int b0 = slice * (rows_per / 32), b1 = min(HW / 32, b0 + rows_per / 32);
    const long base = (long)n * (HW / 32);
    for (int i = threadIdx.x; i < (b1 - b0) * cpg; i += 256) {
      const int b = b0 + i / cpg, c = g * cpg + i % cpg;
      s += (double)stats[(base + b) * C + c];
      ss += (double)stats[stats_plane + (base + b) * C + c];
    }
  } else {
    const int r0 = slice * rows_per, r1 = min(HW, r0 + rows_per);
    const float* xs = x + ((long)n * HW) * C + g * cpg;
    for (int i = threadIdx.x; i < (r1 - r0) * cpg; i += 256) {
      const int r = r0 + i / cpg, c = i % cpg;
      const double v = (double)xs[(long)r * C + c];
      s += v;
      ss += v * v;
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    s += __shfl_xor(s, o);
    ss += __shfl_xor(ss, o);
  }
  if ((threadIdx.x & 63) == 0) {
    red[0][threadIdx.x >> 6] = s;
    red[1][threadIdx.x >> 6] = ss;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double* o = ws + ((long)ng * S + slice) * 2;
    o[0] = (red[0][0] + red[0][1]) + (red[0][2] + red[0][3]);
    o[1] = (red[1][0] + red[1][1]) + (red[1][2] + red[1][3]);
  }
}

struct GaP {
  const float* x; const float* skip; long ld_skip;
  const float* gamma; const float* beta; const double* ws;
  float* y; long ld_y;
  bf16* hi; bf16* lo; long ld_pl;
  int HW, C, G, S, silu, rows_per_block;
  float eps;
};

// block = rows [blockIdx.x * rows_per_block, ..) of sample blockIdx.y; thread = four consecutive channels of one row
__global__ __launch_bounds__(256) void gn_add_apply_kernel(const GaP p) {
  __shared__ float mean_s[GA_MAX_GROUPS], rstd_s[GA_MAX_GROUPS];
  const int n = blockIdx.y, cpg = p.C / p.G;
  if ((int)threadIdx.x < p.G) {
    const double* w = p.ws + ((long)n * p.G + threadIdx.x) * p.S * 2;
    double s = 0.0, ss = 0.0;
    for (int i = 0; i < p.S; ++i) {
      s += w[2 * i];
      ss += w[2 * i + 1];
    }
    const double cnt = (double)p.HW * cpg, mean = s / cnt;
    double var = ss / cnt - mean * mean;
    if (var < 0.0) var = 0.0;
    mean_s[threadIdx.x] = (float)mean;
    rstd_s[threadIdx.x] = (float)(1.0 / sqrt(var + (double)p.eps));
  }
  __syncthreads();
  const int c4 = p.C / 4;
  const int r0 = blockIdx.x * p.rows_per_block, r1 = min(p.HW, r0 + p.rows_per_block);
  for (int i = threadIdx.x; i < (r1 - r0) * c4; i += 256) {
    const int r = r0 + i / c4, c = (i % c4) * 4;
    const long row = (long)n * p.HW + r;
    f32x4 v = *reinterpret_cast<const f32x4*>(p.x + row * p.C + c);
    const f32x4 ga = *reinterpret_cast<const f32x4*>(p.gamma + c), be = *reinterpret_cast<const f32x4*>(p.beta + c);
    f32x4 sk = {0.f, 0.f, 0.f, 0.f};
    if (p.skip) sk = *reinterpret_cast<const f32x4*>(p.skip + row * p.ld_skip + c);
    bf16x4 h4, l4;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int g = (c + e) / cpg;
      float f = __builtin_fmaf((v[e] - mean_s[g]) * rstd_s[g], ga[e], be[e]) + sk[e];
      if (p.silu) f = f / (1.0f + expf(-f));
      v[e] = f;
      const bf16 h = (bf16)f;
      h4[e] = h;
      l4[e] = (bf16)(f - (float)h);
    }
    if (p.y) *reinterpret_cast<f32x4*>(p.y + row * p.ld_y + c) = v;
    if (p.hi) {
      *reinterpret_cast<bf16x4*>(p.hi + row * p.ld_pl + c) = h4;
      *reinterpret_cast<bf16x4*>(p.lo + row * p.ld_pl + c) = l4;
    }
  }
}
int conv_transpose2d_impl(crg_ctx* ctx, void* stream, const crg_conv_transpose_args* a) {
  if (!ctx) return -22;
  ctx->route = crg_route{};
  CRG_REQUIRE(ctx, a && a->x_hi && a->x_lo && a->w_hi && a->w_lo && a->y, "conv_transpose2d: bad arguments");
  CRG_REQUIRE(ctx, a->N >= 1 && a->H >= 1 && a->W >= 1, "conv_transpose2d: empty problem N=%d H=%d W=%d", a->N, a->H, a->W);
  CRG_REQUIRE(ctx, a->Cin >= 8 && a->Cin % 8 == 0 && a->Cout >= 4 && a->Cout % 4 == 0, "conv_transpose2d: Cin=%d must be a multiple of 8, Cout=%d of 4", a->Cin,
              a->Cout);
  const int64_t rows = (int64_t)a->N * a->H * a->W;
  CRG_REQUIRE(ctx, 4 * rows < (1LL << 31) - 128 && (int64_t)16 * a->Cin * a->Cout < (1LL << 40), "conv_transpose2d: %lld source pixels are beyond 2^29",
              (long long)rows);
  CRG_REQUIRE(ctx, (((uintptr_t)a->x_hi | (uintptr_t)a->x_lo | (uintptr_t)a->w_hi | (uintptr_t)a->w_lo | (uintptr_t)a->y | (uintptr_t)a->bias) & 15) == 0,
              "conv_transpose2d: operands must be 16-byte aligned");
  CRG_REQUIRE(ctx, ctx->zero_page, "conv_transpose2d: the context has no zero page");
  {  // y is written while other blocks still read the planes
    const uintptr_t y0 = (uintptr_t)a->y, y1 = y0 + (uintptr_t)rows * 4 * a->Cout * 4, xb = (uintptr_t)rows * a->Cin * sizeof(bf16);
    const uintptr_t h0 = (uintptr_t)a->x_hi, l0 = (uintptr_t)a->x_lo;
    CRG_REQUIRE(ctx, (y1 <= h0 || h0 + xb <= y0) && (y1 <= l0 || l0 + xb <= y0), "conv_transpose2d: y overlaps an activation plane");
  }
  hipStream_t st = (hipStream_t)stream;
  CtP p = {};
  p.x_hi = (const bf16*)a->x_hi; p.x_lo = (const bf16*)a->x_lo; p.w_hi = (const bf16*)a->w_hi; p.w_lo = (const bf16*)a->w_lo;
  p.bias = a->bias; p.y = (float*)a->y; p.zpage = (const bf16*)ctx->zero_page;
  p.M = (int)rows; p.N = a->Cout; p.Cin = a->Cin; p.H = a->H; p.W = a->W; p.silu = a->silu ? 1 : 0;
  p.cm = a->Cin % 64 == 0 ? 1 : 0;  // the K order of CRG_PACK_CONVT_UP2
  p.kchunks = (a->Cin + BK - 1) / BK;
  const int live = (a->H > 1 ? 2 : 1) * (a->W > 1 ? 2 : 1);
  const double flops = 3.0 * 2.0 * 4.0 * rows * p.N * (double)live * a->Cin;  // three matrix passes over the taps walked
  const double bytes = rows * (4.0 * a->Cin + 16.0 * a->Cout) + 4.0 * 4.0 * p.N * (double)live * a->Cin;
  crg_prof_scope ps(ctx, st, CRG_K_CONV_X3, flops, bytes);
  const CtPlan pl = plan_conv_transpose(rows, a->Cout, ctx->n_cu > 0 ? ctx->n_cu : 256);
  ctx->route.kernel = CRG_ROUTE_CONVT;
  ctx->route.wnt = pl.wnt;
  ctx->route.config = pl.wmt;
  ctx->route.splits = 1;
  if (pl.wmt == 1) return launch_conv_transpose<1, 1, 8>(ctx, st, p);
  if (pl.wmt == 2) return launch_conv_transpose<1, 2, 6>(ctx, st, p);
  if (pl.wnt == 4) return launch_conv_transpose<4, 4, 1>(ctx, st, p);
  if (pl.wnt == 2) return launch_conv_transpose<2, 4, 1>(ctx, st, p);
  return launch_conv_transpose<1, 4, 1>(ctx, st, p);
}

int groupnorm_add_act_impl(crg_ctx* ctx, void* stream, const crg_gn_add_act_args* a) {
  if (!ctx) return -22;
  CRG_REQUIRE(ctx, a && a->x && a->gamma && a->beta && a->workspace && (a->y || a->y_hi), "groupnorm_add_act: bad arguments");
  CRG_REQUIRE(ctx, a->N >= 1 && a->HW >= 1 && a->C >= 8 && a->C % 8 == 0, "groupnorm_add_act: N=%d HW=%d C=%d (C must be a multiple of 8)", a->N, a->HW, a->C);
  CRG_REQUIRE(ctx, a->groups >= 1 && a->groups <= GA_MAX_GROUPS && a->C % a->groups == 0, "groupnorm_add_act: %d groups do not divide %d channels (at most %d)",
              a->groups, a->C, GA_MAX_GROUPS);
  CRG_REQUIRE(ctx, (a->y_hi == nullptr) == (a->y_lo == nullptr), "groupnorm_add_act: both planes or none");
  CRG_REQUIRE(ctx, (!a->skip || (a->ld_skip >= a->C && a->ld_skip % 4 == 0)) && (!a->y || (a->ld_y >= a->C && a->ld_y % 4 == 0)) &&
                       (!a->y_hi || (a->ld_planes >= a->C && a->ld_planes % 8 == 0)),
              "groupnorm_add_act: a row stride must cover C and keep rows 16-byte aligned");
  CRG_REQUIRE(ctx, (((uintptr_t)a->x | (uintptr_t)a->skip | (uintptr_t)a->y | (uintptr_t)a->gamma | (uintptr_t)a->beta | (uintptr_t)a->gn_stats) & 15) == 0 &&
                       (((uintptr_t)a->y_hi | (uintptr_t)a->y_lo | (uintptr_t)a->workspace) & 7) == 0,
              "groupnorm_add_act: fp32 operands must be 16-byte aligned, the planes and the workspace 8-byte aligned");
  CRG_REQUIRE(ctx, !a->gn_stats || a->HW % 32 == 0, "groupnorm_add_act: the statistics side channel holds 32-row partials (HW = %d)", a->HW);
  CRG_REQUIRE(ctx, (int64_t)a->N * a->HW < (1LL << 31) && a->N <= 65535, "groupnorm_add_act: N * HW beyond 2^31");
  hipStream_t st = (hipStream_t)stream;
  int S = (a->HW + GA_SLICE_ROWS - 1) / GA_SLICE_ROWS;
  if (S > GA_MAX_SLICES) S = GA_MAX_SLICES;
  int rows_per = (a->HW + S - 1) / S;
  rows_per = (rows_per + 31) / 32 * 32;
  CRG_REQUIRE(ctx, a->workspace_bytes >= (int64_t)a->N * a->groups * S * 16, "groupnorm_add_act: the workspace holds %lld bytes, %lld needed",
              (long long)a->workspace_bytes, (long long)a->N * a->groups * S * 16);
  const double elems = (double)a->N * a->HW * a->C;
  {
    crg_prof_scope ps(ctx, st, CRG_K_GN_STATS, 3.0 * elems, a->gn_stats ? elems / 4 : 4.0 * elems);
    const long plane = (long)((int64_t)a->N * a->HW / 32) * a->C;
    hipLaunchKernelGGL(gn_add_stats_kernel, dim3((unsigned)(a->N * a->groups), (unsigned)S), dim3(256), 0, st, (const float*)a->x, a->gn_stats, plane,
                       (double*)a->workspace, a->HW, a->C, a->groups, S, rows_per);
    CRG_CHECK_LAUNCH(ctx, "groupnorm_add_act (statistics)");
  }
  GaP p = {};
  p.x = (const float*)a->x; p.skip = (const float*)a->skip; p.ld_skip = a->ld_skip;
  p.gamma = a->gamma; p.beta = a->beta; p.ws = (const double*)a->workspace;
  p.y = (float*)a->y; p.ld_y = a->ld_y; p.hi = (bf16*)a->y_hi; p.lo = (bf16*)a->y_lo; p.ld_pl = a->ld_planes;
  p.HW = a->HW; p.C = a->C; p.G = a->groups; p.S = S; p.silu = a->silu ? 1 : 0; p.eps = a->eps;
  // about 2 K elements per block (two 16-byte loads per lane), whole rows: the small images of this network still spread over the CUs
  p.rows_per_block = (2048 + a->C - 1) / a->C;
  const unsigned gx = (unsigned)((a->HW + p.rows_per_block - 1) / p.rows_per_block);
  crg_prof_scope ps(ctx, st, CRG_K_GN_APPLY, 8.0 * elems, elems * (4.0 + (a->skip ? 4.0 : 0.0) + (a->y ? 4.0 : 0.0) + (a->y_hi ? 4.0 : 0.0)));
  hipLaunchKernelGGL(gn_add_apply_kernel, dim3(gx, (unsigned)a->N), dim3(256), 0, st, p);
  CRG_CHECK_LAUNCH(ctx, "groupnorm_add_act");
  return 0;
}
}  // namespace

extern "C" int crg_conv_transpose2d(crg_ctx* ctx, void* stream, const void* x_hi, const void* x_lo, const void* w_hi, const void* w_lo, const float* bias,
                                    void* y, int N, int H, int W, int Cin, int Cout, int silu) {
  const crg_conv_transpose_args a = {x_hi, x_lo, w_hi, w_lo, bias, y, N, H, W, Cin, Cout, silu};
  return conv_transpose2d_impl(ctx, stream, &a);
}

extern "C" int crg_groupnorm_add_act(crg_ctx* ctx, void* stream, const void* x, const void* skip, int64_t ld_skip, const float* gamma, const float* beta,
                                     const float* gn_stats, void* y, int64_t ld_y, void* y_hi, void* y_lo, int64_t ld_planes, void* workspace,
                                     int64_t workspace_bytes, int N, int HW, int C, int groups, float eps, int silu) {
  const crg_gn_add_act_args a = {x, skip, ld_skip, gamma, beta, gn_stats, y, ld_y, y_hi, y_lo, ld_planes, workspace, workspace_bytes, N, HW, C, groups, eps, silu};
  return groupnorm_add_act_impl(ctx, stream, &a);
}
