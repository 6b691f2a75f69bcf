// Temporal layers of the video VAE decoder (sgm temporal_ae.py) on [b][T][S][C] rows - the layout of video.hip.
//
// crg_conv_frames_x3: crg_conv_frames in the fp32 class.  The activation arrives as the two 16-bit planes crg_groupnorm_split /
//   crg_split_bf16 write (hi = half(x), lo = half(x - hi)), the tap-major weight as the two planes of crg_pack_weight; every k-step
//   runs three MFMA passes lo*hi + hi*lo + hi*hi into one fp32 accumulator (the order of gemm_glds_kernel<.., NS = 2>), residual and
//   output are fp32.  Structure of conv_frames_kernel: row m + (tap - 1) S of the SAME plane is the A row of a tap, staged by LDS-DMA in
//   16-byte pieces into the XOR-swizzled 128-byte-row image; a tap whose frame lies outside [0, T) is staged from the context's zero
//   page BY SELECTION - the other video's rows, or rows outside the tensor, are never addressed.  The whole K = 3 Cin of a tile is summed
//   by one block in a fixed order, no split-K, tile width from Cout alone: a row's bits depend on its video and the weights only.
//   LDS: a stage holds four planes, [X hi][X lo][W hi][W lo], 64 KB at the 128 x 128 tile.  Measured: ONE stage and two
//   blocks per CU (128 of the CU's 160 KB) - the DMA of one block's next k-tile runs under the other block's 3 x 32 MFMAs per wave and
//   k-step - is 1.3 - 1.5 x faster than the two-stage ring of gemm_glds_kernel<.., NS = 2> with its one block per CU, and faster
//   than 128 x 64 tiles in either form, at every decoder shape.
//
// crg_conv_frames_thin: the same conv on C <= 8 channels (AE3DConv.time_mix_conv on the 3 pixel channels) - pure HBM traffic, one
//   thread per pixel, fp32 FMAs in a fixed order; frames outside the video are never read.
#include "gemm_shared.h"

namespace {
using crg_mm::BK;
using crg_mm::lds_off;
using crg_mm::wait_vmcnt;
using crg_mm::gptr_t;
using crg_mm::lptr_t;

struct Cf3P {
  const bf16* x_hi; const bf16* x_lo; const bf16* w_hi; const bf16* w_lo;
  const float* bias; const float* cvec; long cvec_ld;
  const float* res; const float* rscale; float* y; const bf16* zpage;
  int M, N, K, Cin, S, T, tiles_n;
};

constexpr int CF_BM = 128;
// one stage of four planes: 64 KB at the 128 x 128 tile, two blocks per CU (DESIGN 6 f17 has the measurement against the two-stage ring)
template <int WNT>
constexpr int cf3_lds_bytes() { return 2 * (CF_BM * 128 + 32 * WNT * 128); }
static_assert(cf3_lds_bytes<4>() == 64 * 1024 && 2 * cf3_lds_bytes<4>() <= 160 * 1024, "four planes at the 128 x 128 tile: 64 KB, two blocks per CU");

template <int WNT>
__global__ __launch_bounds__(256, 2) void conv_frames_x3_kernel(const Cf3P p) {
  constexpr int BN = 32 * WNT, WMT = 4;
  constexpr int XS_BYTES = CF_BM * 128, WS_BYTES = BN * 128;  // the stage: [X hi][X lo][W hi][W lo]
  constexpr int XL = CF_BM / 32, WL = BN / 32;  // 8-row groups (one 1 KiB wave-instruction each) per wave, plane and k-tile
  extern __shared__ __attribute__((aligned(16))) char cf3_smem[];

  const int t = threadIdx.x, lane = t & 63;
  const int wave = __builtin_amdgcn_readfirstlane(t >> 6);
  const int wm = wave >> 1, wn = wave & 1;
  const int tile_n = blockIdx.x % p.tiles_n, tile_m = blockIdx.x / p.tiles_n;
  const int m0 = tile_m * CF_BM, n0 = tile_n * BN;

  // this lane stages LDS row 8 g + lane / 8, physical chunk lane % 8 of row group g = wave + 4 q; it carries logical chunk clog
  const int rsub = lane >> 3, clog = (lane & 7) ^ rsub;
  long xoff[XL];
  bool xprev[XL], xnext[XL], xok[XL];
#pragma unroll
  for (int q = 0; q < XL; ++q) {
    const int m = m0 + (wave + 4 * q) * 8 + rsub;
    const int fr = (m / p.S) % p.T;  // frame of the row inside its video
    xok[q] = m < p.M;
    xprev[q] = fr > 0;
    xnext[q] = fr + 1 < p.T;
    xoff[q] = (long)m * p.Cin;
  }
  long woff[WL];
  bool wok[WL];
#pragma unroll
  for (int q = 0; q < WL; ++q) {
    const int n = n0 + (wave + 4 * q) * 8 + rsub;
    wok[q] = n < p.N;
    woff[q] = (long)n * p.K;
  }
  // running (tap, channel) of this lane's logical chunk (Cin % 32 == 0: an 8-channel chunk never straddles a tap)
  int kc = clog * 8, tap = 0, cch = kc;
  while (cch >= p.Cin) {
    cch -= p.Cin;
    ++tap;
  }
  const long tap_stride = (long)p.S * p.Cin;

  auto stage = [&]() {
    char* xs = cf3_smem;
    char* ws = xs + 2 * XS_BYTES;
    const bool kok = kc < p.K;
#pragma unroll
    for (int q = 0; q < XL; ++q) {
      const bool ok = kok && xok[q] && (tap == 1 || (tap == 0 ? xprev[q] : xnext[q]));
      const long o = xoff[q] + (long)(tap - 1) * tap_stride + cch;  // only added to a plane's base when ok
      const bf16* sh = ok ? p.x_hi + o : p.zpage;
      const bf16* sl = ok ? p.x_lo + o : p.zpage;
      __builtin_amdgcn_global_load_lds((gptr_t)sh, (lptr_t)(xs + (wave + 4 * q) * 1024), 16, 0, 0);
      __builtin_amdgcn_global_load_lds((gptr_t)sl, (lptr_t)(xs + XS_BYTES + (wave + 4 * q) * 1024), 16, 0, 0);
    }
#pragma unroll
    for (int q = 0; q < WL; ++q) {
      const bool ok = kok && wok[q];
      const bf16* sh = ok ? p.w_hi + woff[q] + kc : p.zpage;
      const bf16* sl = ok ? p.w_lo + woff[q] + kc : p.zpage;
      __builtin_amdgcn_global_load_lds((gptr_t)sh, (lptr_t)(ws + (wave + 4 * q) * 1024), 16, 0, 0);
      __builtin_amdgcn_global_load_lds((gptr_t)sl, (lptr_t)(ws + WS_BYTES + (wave + 4 * q) * 1024), 16, 0, 0);
    }
    kc += BK;
    cch += BK;
    while (cch >= p.Cin) {
      cch -= p.Cin;
      ++tap;
    }
  };

  f32x4 acc[WNT][WMT];
#pragma unroll
  for (int i = 0; i < WNT; ++i)
#pragma unroll
    for (int j = 0; j < WMT; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  const int frow = lane & 15, fq = lane >> 4;

  const int nk = (p.K + BK - 1) / BK;
  stage();
  const char* xs = cf3_smem;
  const char* ws = xs + 2 * XS_BYTES;
  for (int kt = 0; kt < nk; ++kt) {
    wait_vmcnt<0>();
    asm volatile("" ::: "memory");
    __builtin_amdgcn_s_barrier();  // k-tile kt has landed for every wave
    asm volatile("" ::: "memory");
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      bf16x8 xf[WMT], xl[WMT], wf[WNT], wl[WNT];
#pragma unroll
      for (int j = 0; j < WMT; ++j) {
        const int off = lds_off(wm * 64 + j * 16 + frow, ks * 4 + fq);
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
        for (int j = 0; j < WMT; ++j) {  // the small products first, as in gemm_glds_kernel<.., NS = 2>
          acc[i][j] = CRG_MFMA_16x16x32(wl[i], xf[j], acc[i][j]);
          acc[i][j] = CRG_MFMA_16x16x32(wf[i], xl[j], acc[i][j]);
          acc[i][j] = CRG_MFMA_16x16x32(wf[i], xf[j], acc[i][j]);
        }
    }
    asm volatile("" ::: "memory");
    __builtin_amdgcn_s_barrier();  // everybody is done reading before the next k-tile overwrites the stage; the other block of the CU
    asm volatile("" ::: "memory");  // runs its MFMAs under this one's DMA
    if (kt + 1 < nk) stage();
  }

  // lane: row m = .. + frow, output channels n .. n + 3 of each 16 x 16 tile (N % 32 == 0: a group of four is in or out as a whole).
  // y may alias the residual: a lane reads its own 16 bytes before it writes them, and no other lane touches them
#pragma unroll
  for (int j = 0; j < WMT; ++j) {
    const int m = m0 + wm * 64 + j * 16 + frow;
    if (m >= p.M) continue;
    const int frame = m / p.S;
    const float rs = p.rscale ? p.rscale[frame] : 1.0f;
    const float* cv = p.cvec ? p.cvec + (long)frame * p.cvec_ld : nullptr;
#pragma unroll
    for (int i = 0; i < WNT; ++i) {
      const int n = n0 + wn * (16 * WNT) + i * 16 + fq * 4;
      if (n >= p.N) continue;
      f32x4 v = acc[i][j];
      if (p.bias) v += *reinterpret_cast<const f32x4*>(p.bias + n);
      if (cv) v += *reinterpret_cast<const f32x4*>(cv + n);
      const long yo = (long)m * p.N + n;
      if (p.res) {
        const f32x4 r4 = *reinterpret_cast<const f32x4*>(p.res + yo);
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = __builtin_fmaf(rs, v[e], r4[e]);
      }
      *reinterpret_cast<f32x4*>(p.y + yo) = v;
    }
  }
}

template <int WNT>
int launch_conv_frames_x3(crg_ctx* ctx, hipStream_t st, Cf3P& p) {
  const void* kern = reinterpret_cast<const void*>(&conv_frames_x3_kernel<WNT>);
  if (int rc = crg_set_dyn_lds(ctx, kern, cf3_lds_bytes<WNT>(), "conv_frames_x3")) return rc;
  p.tiles_n = (p.N + 32 * WNT - 1) / (32 * WNT);
  const long tiles = (long)((p.M + CF_BM - 1) / CF_BM) * p.tiles_n;
  if (tiles > 0x7fffffffL) return crg_fail(ctx, -22, "conv_frames_x3: %ld tiles exceed the grid", tiles);
  hipLaunchKernelGGL((conv_frames_x3_kernel<WNT>), dim3((unsigned)tiles), dim3(256), cf3_lds_bytes<WNT>(), st, p);
  CRG_CHECK_LAUNCH(ctx, "conv_frames_x3");
  return 0;
}

// ---- thin frame conv -----------------------------------------------------------------------------------------------------------
struct CftP {
  const void* x; const float* w; const float* bias; void* y;
  long M;
  int C, S, T;
};

// One thread per pixel row m.  CP: instantiated channel count >= C.  The block's copy of the weights is laid out [tap][co][ci] in LDS
// (every lane reads the same word: a broadcast).  y[m][co] = bias[co], then for tap d = -1, 0, 1 (skipped as a whole when frame t + d is
// outside the video) and ci = 0 .. C - 1:  y = fma(w[co][ci][d], x[m + d S][ci], y).
template <typename TT, int CP>
__global__ __launch_bounds__(256) void conv_frames_thin_kernel(const CftP p) {
  __shared__ float wsm[3 * CP * CP];
  __shared__ float bsm[CP];
  const int C = p.C;
  for (int i = threadIdx.x; i < 3 * CP * CP; i += 256) {
    const int d = i / (CP * CP), r = i - d * CP * CP, co = r / CP, ci = r - co * CP;
    wsm[i] = (co < C && ci < C) ? p.w[(co * C + ci) * 3 + d] : 0.f;
  }
  if (threadIdx.x < CP) bsm[threadIdx.x] = (p.bias && (int)threadIdx.x < C) ? p.bias[threadIdx.x] : 0.f;
  __syncthreads();
  const long m = (long)blockIdx.x * 256 + threadIdx.x;
  if (m >= p.M) return;  // no barrier below
  const int fr = (int)((m / p.S) % p.T);
  const TT* X = reinterpret_cast<const TT*>(p.x);
  float acc[CP];
#pragma unroll
  for (int co = 0; co < CP; ++co) acc[co] = bsm[co];
#pragma unroll
  for (int d = 0; d < 3; ++d) {
    const bool in = d == 1 || (d == 0 ? fr > 0 : fr + 1 < p.T);
    if (!in) continue;  // the row m + (d - 1) S belongs to another video or lies outside the tensor: never addressed
    const TT* xr = X + (m + (long)(d - 1) * p.S) * C;
    float xv[CP];
#pragma unroll
    for (int ci = 0; ci < CP; ++ci) xv[ci] = ci < C ? (float)xr[ci] : 0.f;
#pragma unroll
    for (int ci = 0; ci < CP; ++ci) {
      if (ci < C) {
#pragma unroll
        for (int co = 0; co < CP; ++co) acc[co] = __builtin_fmaf(wsm[(d * CP + co) * CP + ci], xv[ci], acc[co]);
      }
    }
  }
  TT* Y = reinterpret_cast<TT*>(p.y) + m * C;
#pragma unroll
  for (int co = 0; co < CP; ++co)
    if (co < C) Y[co] = (TT)acc[co];
}

template <typename TT>
int launch_conv_frames_thin(crg_ctx* ctx, hipStream_t st, const CftP& p) {
  const dim3 grid((unsigned)((p.M + 255) / 256));
  if (p.C <= 4)
    hipLaunchKernelGGL((conv_frames_thin_kernel<TT, 4>), grid, dim3(256), 0, st, p);
  else
    hipLaunchKernelGGL((conv_frames_thin_kernel<TT, 8>), grid, dim3(256), 0, st, p);
  CRG_CHECK_LAUNCH(ctx, "conv_frames_thin");
  return 0;
}
}  // namespace

extern "C" int crg_conv_frames_x3(crg_ctx* ctx, void* stream, const crg_conv_frames_x3_args* a) {
  if (!ctx) return -22;
  CRG_REQUIRE(ctx, a && a->x_hi && a->x_lo && a->w_hi && a->w_lo && a->y, "conv_frames_x3: bad arguments");
  CRG_REQUIRE(ctx, a->b >= 1 && a->T >= 1 && a->S >= 1, "conv_frames_x3: empty problem b=%d T=%d S=%d", a->b, a->T, a->S);
  CRG_REQUIRE(ctx, a->Cin >= 32 && a->Cin % 32 == 0 && a->Cout >= 32 && a->Cout % 32 == 0,
              "conv_frames_x3: Cin=%d / Cout=%d must be multiples of 32", a->Cin, a->Cout);
  const int64_t rows = (int64_t)a->b * a->T * a->S;
  CRG_REQUIRE(ctx, rows < (1LL << 31) - CF_BM && (int64_t)3 * a->Cin < (1LL << 31), "conv_frames_x3: %lld rows are beyond 2^31", (long long)rows);
  CRG_REQUIRE(ctx, !a->rscale || a->residual, "conv_frames_x3: rscale needs a residual");
  CRG_REQUIRE(ctx, !a->cvec || (a->cvec_ld >= a->Cout && a->cvec_ld % 4 == 0), "conv_frames_x3: cvec_ld=%lld must cover Cout and be a multiple of 4",
              (long long)a->cvec_ld);
  CRG_REQUIRE(ctx, (((uintptr_t)a->x_hi | (uintptr_t)a->x_lo | (uintptr_t)a->w_hi | (uintptr_t)a->w_lo | (uintptr_t)a->y | (uintptr_t)a->residual |
                     (uintptr_t)a->bias | (uintptr_t)a->cvec) & 15) == 0,
              "conv_frames_x3: operands must be 16-byte aligned");
  CRG_REQUIRE(ctx, ctx->zero_page, "conv_frames_x3: the context has no zero page");
  {  // y is written while other blocks still read the planes: it must not overlap them (it may BE the residual)
    const uintptr_t y0 = (uintptr_t)a->y, y1 = y0 + (uintptr_t)rows * a->Cout * 4, xb = (uintptr_t)rows * a->Cin * sizeof(bf16);
    const uintptr_t h0 = (uintptr_t)a->x_hi, l0 = (uintptr_t)a->x_lo;
    CRG_REQUIRE(ctx, (y1 <= h0 || h0 + xb <= y0) && (y1 <= l0 || l0 + xb <= y0), "conv_frames_x3: y overlaps an activation plane");
    CRG_REQUIRE(ctx, !a->residual || a->residual == a->y || (uintptr_t)a->residual + (y1 - y0) <= y0 || y1 <= (uintptr_t)a->residual,
                "conv_frames_x3: y overlaps the residual at an offset (it may alias it exactly)");
  }
  hipStream_t st = (hipStream_t)stream;
  Cf3P p = {};
  p.x_hi = (const bf16*)a->x_hi; p.x_lo = (const bf16*)a->x_lo; p.w_hi = (const bf16*)a->w_hi; p.w_lo = (const bf16*)a->w_lo;
  p.bias = a->bias; p.cvec = a->cvec; p.cvec_ld = a->cvec_ld;
  p.res = (const float*)a->residual; p.rscale = a->rscale; p.y = (float*)a->y; p.zpage = (const bf16*)ctx->zero_page;
  p.M = (int)rows; p.N = a->Cout; p.K = 3 * a->Cin; p.Cin = a->Cin; p.S = a->S; p.T = a->T;
  const double flops = 3.0 * 2.0 * rows * p.N * p.K;  // three matrix passes
  const double bytes = rows * (4.0 * a->Cin + (a->residual ? 8.0 : 4.0) * a->Cout) + 4.0 * p.N * p.K;
  crg_prof_scope ps(ctx, st, CRG_K_GEMM_X3, flops, bytes);
  // tile width from Cout alone (never from b): the widest of 128 / 64 / 32 that divides it
  if (p.N % 128 == 0) return launch_conv_frames_x3<4>(ctx, st, p);
  if (p.N % 64 == 0) return launch_conv_frames_x3<2>(ctx, st, p);
  return launch_conv_frames_x3<1>(ctx, st, p);
}

extern "C" int crg_conv_frames_thin(crg_ctx* ctx, void* stream, const void* x, const float* w, const float* bias, void* y, int b, int T, int S,
                                    int C, int dtype) {
  if (!ctx) return -22;
  CRG_REQUIRE(ctx, x && w && y, "conv_frames_thin: bad arguments");
  CRG_REQUIRE(ctx, b >= 1 && T >= 1 && S >= 1, "conv_frames_thin: empty problem b=%d T=%d S=%d", b, T, S);
  CRG_REQUIRE(ctx, C >= 1 && C <= 8, "conv_frames_thin: C=%d channels unsupported (1 .. 8)", C);
  CRG_REQUIRE(ctx, dtype == CRG_BF16 || dtype == CRG_F32, "conv_frames_thin: dtype %d unsupported", dtype);
  const int64_t rows = (int64_t)b * T * S;
  {  // a pixel reads its neighbour frames, which another block may already have written: no overlap at any offset
    const uintptr_t n = (uintptr_t)rows * C * crg_dtype_size(dtype), x0 = (uintptr_t)x, y0 = (uintptr_t)y;
    CRG_REQUIRE(ctx, x0 + n <= y0 || y0 + n <= x0, "conv_frames_thin: y must not overlap x (a pixel reads its neighbour frames)");
  }
  CRG_REQUIRE(ctx, (rows + 255) / 256 < (1LL << 31), "conv_frames_thin: %lld rows exceed the grid", (long long)rows);
  hipStream_t st = (hipStream_t)stream;
  CftP p = {x, w, bias, y, (long)rows, C, S, T};
  crg_prof_scope ps(ctx, st, CRG_K_ELEMENTWISE, 2.0 * rows * 3 * C * C, 2.0 * rows * C * crg_dtype_size(dtype));
  return dtype == CRG_F32 ? launch_conv_frames_thin<float>(ctx, st, p) : launch_conv_frames_thin<bf16>(ctx, st, p);
}
