// Temporal layers of the video UNet (sgm video_model.py / video_attention.py) on activations that stay [(b t), h, w, c] channels-last,
// i.e. the same bytes as [b][T][S][C] with S = h w: the reference's (b t) s c <-> (b s) t c rearranges are index arithmetic here.
//
// crg_conv_frames: the (3, 1, 1) conv along the frame axis (VideoResBlock.time_stack) as an implicit GEMM with K = 3 Cin, tap-major.
//   Row m = (v T + t) S + s of the [b T S][Cin] activation matrix; the A row of tap d (d = -1, 0, 1) is row m + d S of the SAME matrix,
//   so a k-tile is staged by LDS-DMA from a row offset - no im2col tensor.  A tap whose frame t + d lies outside [0, T) is staged from the
//   context's zero page BY SELECTION: the row m + d S, which belongs to another video or lies outside the tensor, is never addressed.
//   128-row x (32 WNT)-column tiles, four waves 2 x 2, 64-deep k-tiles in a two-stage ring, 16x16x32 MFMA with the weight tile as the A
//   operand (a lane then owns four consecutive output channels of one row: 8-byte epilogue accesses) - the geometry of gemm_glds_kernel's
//   configuration A.  The whole K of an output tile is summed by one block in a fixed order and the tile width is a function of Cout
//   alone: the bits of a row depend on its video and the weights only, never on b (batch-invariant with the mode on or off).
//   Epilogue: + bias[n] + cvec[frame][n], then y = residual + rscale[frame] * y.
//
// crg_attention_frames: softmax(q k^T scale) v over the T <= 32 frames of each (video, pixel, head), on the vector unit.  One thread
//   owns one query row (frame t of a (pixel, head) group); a block of 256 threads owns G = 256 / T groups, numbered head-fastest, so
//   that a block covers whole token rows (all heads) of adjacent pixels.  The K and V rows of the block's groups are staged in LDS in
//   16-byte pieces (eight consecutive lanes fetch one 128-byte row) and every thread of a group reads them as LDS broadcasts; q k^T, the
//   softmax and p v are fp32 FMAs in registers.  Why not MFMA: at T = 25 and d = 64 a (pixel, head) problem is 0.16 MFLOP against 9.6 KB
//   of traffic; the p v product needs V with the frame index innermost, i.e. a transpose through LDS per problem, while the whole
//   launch is ~15 GFLOP - about the time of its four passes over HBM on the vector unit already.  Videos never share a block.
//
// crg_add_frames / crg_lincomb_frames: per-frame channel vector added to tokens; y = a[frame] x + c[frame] z.
#include "gemm_shared.h"

namespace {
using crg_mm::BK;
using crg_mm::lds_off;
using crg_mm::wait_vmcnt;
using crg_mm::gptr_t;
using crg_mm::lptr_t;

struct CfP {
  const bf16* x; const bf16* w; const float* bias; const float* cvec; long cvec_ld;
  const bf16* res; const float* rscale; bf16* y; const bf16* zpage;
  int M, N, K, Cin, S, T, tiles_n;
};

constexpr int CF_BM = 128;
template <int WNT>
constexpr int cf_lds_bytes() { return 2 * (CF_BM * 128 + 32 * WNT * 128); }

template <int WNT>
__global__ __launch_bounds__(256, 2) void conv_frames_kernel(const CfP p) {
  constexpr int BN = 32 * WNT, WMT = 4;
  constexpr int XS_BYTES = CF_BM * 128, STAGE_BYTES = XS_BYTES + BN * 128;
  constexpr int XL = CF_BM / 32, WL = BN / 32;  // 8-row groups (one 1 KiB wave-instruction each) per wave and k-tile
  extern __shared__ __attribute__((aligned(16))) char cf_smem[];

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

  auto stage = [&](int buf) {
    char* xs = cf_smem + buf * STAGE_BYTES;
    char* ws = xs + XS_BYTES;
    const bool kok = kc < p.K;
#pragma unroll
    for (int q = 0; q < XL; ++q) {
      const bool ok = kok && xok[q] && (tap == 1 || (tap == 0 ? xprev[q] : xnext[q]));
      const bf16* src = ok ? p.x + xoff[q] + (long)(tap - 1) * tap_stride + cch : p.zpage;
      __builtin_amdgcn_global_load_lds((gptr_t)src, (lptr_t)(xs + (wave + 4 * q) * 1024), 16, 0, 0);
    }
#pragma unroll
    for (int q = 0; q < WL; ++q) {
      const bf16* src = (kok && wok[q]) ? p.w + woff[q] + kc : p.zpage;
      __builtin_amdgcn_global_load_lds((gptr_t)src, (lptr_t)(ws + (wave + 4 * q) * 1024), 16, 0, 0);
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
  stage(0);
  int buf = 0;
  for (int kt = 0; kt < nk; ++kt) {
    wait_vmcnt<0>();
    asm volatile("" ::: "memory");
    __builtin_amdgcn_s_barrier();  // k-tile kt has landed for every wave; nobody reads the other buffer any more
    asm volatile("" ::: "memory");
    if (kt + 1 < nk) stage(buf ^ 1);
    const char* xs = cf_smem + buf * STAGE_BYTES;
    const char* ws = xs + XS_BYTES;
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
      bf16x8 xf[WMT], wf[WNT];
#pragma unroll
      for (int j = 0; j < WMT; ++j) xf[j] = *reinterpret_cast<const bf16x8*>(xs + lds_off(wm * 64 + j * 16 + frow, ks * 4 + fq));
#pragma unroll
      for (int i = 0; i < WNT; ++i) wf[i] = *reinterpret_cast<const bf16x8*>(ws + lds_off(wn * (16 * WNT) + i * 16 + frow, ks * 4 + fq));
#pragma unroll
      for (int i = 0; i < WNT; ++i)
#pragma unroll
        for (int j = 0; j < WMT; ++j) acc[i][j] = CRG_MFMA_16x16x32(wf[i], xf[j], acc[i][j]);
    }
    buf ^= 1;
  }

  // lane: row m = .. + frow, output channels n .. n + 3 of each 16 x 16 tile (N % 32 == 0: a group of four is in or out as a whole)
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
        const bf16x4 r4 = *reinterpret_cast<const bf16x4*>(p.res + yo);
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] = __builtin_fmaf(rs, v[e], (float)r4[e]);
      }
      bf16x4 o4;
#pragma unroll
      for (int e = 0; e < 4; ++e) o4[e] = (bf16)v[e];
      *reinterpret_cast<bf16x4*>(p.y + yo) = o4;
    }
  }
}

template <int WNT>
int launch_conv_frames(crg_ctx* ctx, hipStream_t st, CfP& p) {
  const void* kern = reinterpret_cast<const void*>(&conv_frames_kernel<WNT>);
  if (int rc = crg_set_dyn_lds(ctx, kern, cf_lds_bytes<WNT>(), "conv_frames")) return rc;
  p.tiles_n = (p.N + 32 * WNT - 1) / (32 * WNT);
  const long tiles = (long)((p.M + CF_BM - 1) / CF_BM) * p.tiles_n;
  if (tiles > 0x7fffffffL) return crg_fail(ctx, -22, "conv_frames: %ld tiles exceed the grid", tiles);
  hipLaunchKernelGGL((conv_frames_kernel<WNT>), dim3((unsigned)tiles), dim3(256), cf_lds_bytes<WNT>(), st, p);
  CRG_CHECK_LAUNCH(ctx, "conv_frames");
  return 0;
}

// ---- attention across frames ---------------------------------------------------------------------------------------------------
constexpr int AF_MAX_T = 32;

// TT: element type of q, k, v and o.  DP: instantiated head width >= Dh.  sl2 = scale * log2(e).  G: (pixel, head) groups per block.
template <typename TT, int DP>
__global__ __launch_bounds__(256) void attn_frames_kernel(const crg_attn_frames_args p, const float sl2, const int G) {
  constexpr int ROWB = DP * (int)sizeof(TT) + 16;  // LDS row: the head's channels + 16 bytes (group strides off a common bank)
  constexpr int PCS = DP / 8;
  extern __shared__ __attribute__((aligned(16))) char af_smem[];
  const int T = p.T, S = p.S, H = p.H, Dh = p.Dh, SH = S * H;
  const int rows = G * T;
  char* const ks = af_smem;
  char* const vs = af_smem + rows * ROWB;
  const int tid = threadIdx.x, vb = blockIdx.y, g0 = blockIdx.x * G;
  const TT* const Q = reinterpret_cast<const TT*>(p.q);
  const TT* const K = reinterpret_cast<const TT*>(p.k);
  const TT* const V = reinterpret_cast<const TT*>(p.v);

  // this thread's query row
  const int g = tid / T, t = tid - g * T, gg = g0 + g;
  const bool active = g < G && gg < SH;
  const int px = active ? gg / H : 0, hd = active ? gg - px * H : 0;
  const long qrow = ((long)vb * T + t) * S + px;  // inactive threads: never dereferenced
  crg_vec8<TT> qv[PCS];
  if (active) {
#pragma unroll
    for (int c = 0; c < PCS; ++c)
      if (c * 8 < Dh) qv[c].load(Q + qrow * p.ldq + hd * Dh + c * 8);
  }

  // K and V rows of the block's groups -> LDS, in 16-byte pieces (consecutive threads: consecutive pieces of one row)
  const int ppr = Dh * (int)sizeof(TT) / 16;
  constexpr int EPP = 16 / (int)sizeof(TT);
  for (int i = tid; i < rows * ppr; i += 256) {
    const int row = i / ppr, pc = i - row * ppr;
    const int rg = row / T, rt = row - rg * T, rgg = g0 + rg;
    if (rgg < SH) {
      const int rpx = rgg / H, rhd = rgg - rpx * H;
      const long r = ((long)vb * T + rt) * S + rpx;
      const uint4 kk = *reinterpret_cast<const uint4*>(K + r * p.ldk + rhd * Dh + pc * EPP);
      const uint4 vv = *reinterpret_cast<const uint4*>(V + r * p.ldv + rhd * Dh + pc * EPP);
      *reinterpret_cast<uint4*>(ks + row * ROWB + pc * 16) = kk;
      *reinterpret_cast<uint4*>(vs + row * ROWB + pc * 16) = vv;
    }
  }
  __syncthreads();
  if (!active) return;  // no barrier below

  const char* const kg = ks + g * T * ROWB;
  const char* const vg = vs + g * T * ROWB;
  float s[AF_MAX_T];
  float mx = -__builtin_inff();
#pragma unroll
  for (int j = 0; j < AF_MAX_T; ++j) {
    s[j] = -__builtin_inff();
    if (j < T) {
      float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
#pragma unroll
      for (int c = 0; c < PCS; ++c) {
        if (c * 8 < Dh) {
          crg_vec8<TT> kv;
          kv.load(reinterpret_cast<const TT*>(kg + j * ROWB) + c * 8);
          a0 = __builtin_fmaf(qv[c].get(0), kv.get(0), a0);
          a1 = __builtin_fmaf(qv[c].get(1), kv.get(1), a1);
          a2 = __builtin_fmaf(qv[c].get(2), kv.get(2), a2);
          a3 = __builtin_fmaf(qv[c].get(3), kv.get(3), a3);
          a0 = __builtin_fmaf(qv[c].get(4), kv.get(4), a0);
          a1 = __builtin_fmaf(qv[c].get(5), kv.get(5), a1);
          a2 = __builtin_fmaf(qv[c].get(6), kv.get(6), a2);
          a3 = __builtin_fmaf(qv[c].get(7), kv.get(7), a3);
        }
      }
      s[j] = ((a0 + a1) + (a2 + a3)) * sl2;
      mx = __builtin_fmaxf(mx, s[j]);
    }
  }
  float l = 0.f;
#pragma unroll
  for (int j = 0; j < AF_MAX_T; ++j) {
    s[j] = j < T ? __builtin_amdgcn_exp2f(s[j] - mx) : 0.f;  // frames >= T: zero by selection
    l += s[j];
  }
  float o[DP];
#pragma unroll
  for (int e = 0; e < DP; ++e) o[e] = 0.f;
#pragma unroll
  for (int j = 0; j < AF_MAX_T; ++j) {
    if (j < T) {
#pragma unroll
      for (int c = 0; c < PCS; ++c) {
        if (c * 8 < Dh) {
          crg_vec8<TT> vv;
          vv.load(reinterpret_cast<const TT*>(vg + j * ROWB) + c * 8);
#pragma unroll
          for (int e = 0; e < 8; ++e) o[c * 8 + e] = __builtin_fmaf(s[j], vv.get(e), o[c * 8 + e]);
        }
      }
    }
  }
  const float inv = 1.0f / l;  // l >= 1 (the maximum's own term); T = 1: exactly 1, the output is V
  TT* const O = reinterpret_cast<TT*>(p.o) + qrow * p.ldo + hd * Dh;
#pragma unroll
  for (int c = 0; c < PCS; ++c) {
    if (c * 8 < Dh) {
      crg_vec8<TT> ov;
#pragma unroll
      for (int e = 0; e < 8; ++e) ov.set(e, o[c * 8 + e] * inv);
      ov.store(O + c * 8);
    }
  }
}

template <typename TT, int DP>
int launch_attn_frames(crg_ctx* ctx, hipStream_t st, const crg_attn_frames_args& a) {
  const int G = 256 / a.T;
  const size_t lds = (size_t)2 * G * a.T * (DP * sizeof(TT) + 16);
  const void* kern = reinterpret_cast<const void*>(&attn_frames_kernel<TT, DP>);
  if (int rc = crg_set_dyn_lds(ctx, kern, (size_t)2 * 256 * (DP * sizeof(TT) + 16), "attention_frames")) return rc;
  const long groups = (long)a.S * a.H;
  const dim3 grid((unsigned)((groups + G - 1) / G), a.b);
  hipLaunchKernelGGL((attn_frames_kernel<TT, DP>), grid, dim3(256), lds, st, a, a.scale * 1.4426950408889634f, G);
  CRG_CHECK_LAUNCH(ctx, "attention_frames");
  return 0;
}

template <typename TT>
int dispatch_attn_frames(crg_ctx* ctx, hipStream_t st, const crg_attn_frames_args& a) {
  if (a.Dh <= 16) return launch_attn_frames<TT, 16>(ctx, st, a);
  if (a.Dh <= 32) return launch_attn_frames<TT, 32>(ctx, st, a);
  return launch_attn_frames<TT, 64>(ctx, st, a);
}

// ---- per-frame elementwise -----------------------------------------------------------------------------------------------------
// y[r][c] = x[r][c] + e[r / S][c]; n8 = rows * C / 8 groups of eight channels
template <typename TT>
__global__ __launch_bounds__(256) void add_frames_kernel(const TT* x, const TT* e, TT* y, long n8, int c8, int S) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n8) return;
  const long r = i / c8;
  const int c = (int)(i - r * c8);
  crg_vec8<TT> xv, ev;
  xv.load(x + i * 8);
  ev.load(e + ((r / S) * c8 + c) * 8);
#pragma unroll
  for (int k = 0; k < 8; ++k) xv.set(k, xv.get(k) + ev.get(k));
  xv.store(y + i * 8);
}

// y = a[frame] x + c[frame] z, each product and the sum rounded on its own in fp32 (what the framework's a * x + c * z gives on fp32
// tensors; no contraction into an FMA); a or c NULL = 1, its product is skipped
template <typename TT>
__global__ __launch_bounds__(256) void lincomb_frames_kernel(const float* a, const TT* x, const float* c, const TT* z, TT* y, long n8, long per_frame8) {
  const long i = (long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n8) return;
  const long f = i / per_frame8;
  const float af = a ? a[f] : 1.0f, cf = c ? c[f] : 1.0f;
  crg_vec8<TT> xv, zv;
  xv.load(x + i * 8);
  zv.load(z + i * 8);
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const float u = a ? __fmul_rn(af, xv.get(k)) : xv.get(k);
    const float w = c ? __fmul_rn(cf, zv.get(k)) : zv.get(k);
    xv.set(k, __fadd_rn(u, w));
  }
  xv.store(y + i * 8);
}

inline unsigned ew_grid(long n8) { return (unsigned)((n8 + 255) / 256); }
}  // namespace

extern "C" int crg_conv_frames(crg_ctx* ctx, void* stream, const crg_conv_frames_args* a) {
  if (!ctx) return -22;
  CRG_REQUIRE(ctx, a && a->x && a->w && a->y, "conv_frames: bad arguments");
  CRG_REQUIRE(ctx, a->b >= 1 && a->T >= 1 && a->S >= 1, "conv_frames: empty problem b=%d T=%d S=%d", a->b, a->T, a->S);
  CRG_REQUIRE(ctx, a->Cin >= 32 && a->Cin % 32 == 0 && a->Cout >= 32 && a->Cout % 32 == 0,
              "conv_frames: Cin=%d / Cout=%d must be multiples of 32", a->Cin, a->Cout);
  const int64_t rows = (int64_t)a->b * a->T * a->S;
  CRG_REQUIRE(ctx, rows < (1LL << 31) - CF_BM && (int64_t)3 * a->Cin < (1LL << 31), "conv_frames: %lld rows are beyond 2^31", (long long)rows);
  CRG_REQUIRE(ctx, !a->rscale || a->residual, "conv_frames: rscale needs a residual");
  CRG_REQUIRE(ctx, !a->cvec || (a->cvec_ld >= a->Cout && a->cvec_ld % 4 == 0), "conv_frames: cvec_ld=%lld must cover Cout and be a multiple of 4",
              (long long)a->cvec_ld);
  CRG_REQUIRE(ctx, (((uintptr_t)a->x | (uintptr_t)a->w | (uintptr_t)a->y | (uintptr_t)a->residual | (uintptr_t)a->bias | (uintptr_t)a->cvec) & 15) == 0,
              "conv_frames: operands must be 16-byte aligned");
  CRG_REQUIRE(ctx, ctx->zero_page, "conv_frames: the context has no zero page");
  hipStream_t st = (hipStream_t)stream;
  CfP p = {};
  p.x = (const bf16*)a->x; p.w = (const bf16*)a->w; p.bias = a->bias; p.cvec = a->cvec; p.cvec_ld = a->cvec_ld;
  p.res = (const bf16*)a->residual; p.rscale = a->rscale; p.y = (bf16*)a->y; p.zpage = (const bf16*)ctx->zero_page;
  p.M = (int)rows; p.N = a->Cout; p.K = 3 * a->Cin; p.Cin = a->Cin; p.S = a->S; p.T = a->T;
  const double flops = 2.0 * rows * p.N * p.K;
  const double bytes = 2.0 * (rows * (double)(a->Cin + (a->residual ? 2 : 1) * a->Cout) + (double)p.N * p.K);
  // tile width from Cout alone (never from b): the widest of 128 / 64 / 32 that divides it
  if (p.N % 128 == 0) {
    crg_prof_scope ps(ctx, st, CRG_K_CONV_W4, flops, bytes);
    return launch_conv_frames<4>(ctx, st, p);
  }
  crg_prof_scope ps(ctx, st, CRG_K_CONV_W1, flops, bytes);
  if (p.N % 64 == 0) return launch_conv_frames<2>(ctx, st, p);
  return launch_conv_frames<1>(ctx, st, p);
}

extern "C" int crg_attention_frames(crg_ctx* ctx, void* stream, const crg_attn_frames_args* a) {
  if (!ctx) return -22;
  CRG_REQUIRE(ctx, a && a->q && a->k && a->v && a->o, "attention_frames: bad arguments");
  CRG_REQUIRE(ctx, a->b >= 1 && a->T >= 1 && a->S >= 1 && a->H >= 1, "attention_frames: empty problem b=%d T=%d S=%d H=%d", a->b, a->T, a->S, a->H);
  CRG_REQUIRE(ctx, a->T <= AF_MAX_T, "attention_frames: T=%d frames unsupported (at most %d)", a->T, AF_MAX_T);
  CRG_REQUIRE(ctx, a->Dh % 8 == 0 && a->Dh >= 8 && a->Dh <= 64, "attention_frames: head dim %d unsupported (multiple of 8, 8 .. 64)", a->Dh);
  CRG_REQUIRE(ctx, a->dtype == CRG_BF16 || a->dtype == CRG_F32, "attention_frames: dtype %d unsupported", a->dtype);
  CRG_REQUIRE(ctx, a->b <= 65535, "attention_frames: b=%d beyond the grid's 65535", a->b);
  const int64_t width = (int64_t)a->H * a->Dh, rows = (int64_t)a->b * a->T * a->S, groups = (int64_t)a->S * a->H;
  CRG_REQUIRE(ctx, rows < (1LL << 31) && groups < (1LL << 31) - 256, "attention_frames: %lld rows are beyond 2^31", (long long)rows);
  CRG_REQUIRE(ctx, a->ldq >= width && a->ldk >= width && a->ldv >= width && a->ldo >= width,
              "attention_frames: ldq / ldk / ldv / ldo must cover H*Dh=%lld", (long long)width);
  const int64_t al = 16 / (int64_t)crg_dtype_size(a->dtype);
  CRG_REQUIRE(ctx, a->ldq % al == 0 && a->ldk % al == 0 && a->ldv % al == 0 && a->ldo % al == 0,
              "attention_frames: row strides must keep 16-byte alignment (multiples of %lld)", (long long)al);
  CRG_REQUIRE(ctx, (((uintptr_t)a->q | (uintptr_t)a->k | (uintptr_t)a->v | (uintptr_t)a->o) & 15) == 0, "attention_frames: q, k, v and o must be 16-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  const double flops = 4.0 * rows * a->T * width;
  const double bytes = 4.0 * rows * width * crg_dtype_size(a->dtype);
  crg_prof_scope ps(ctx, st, CRG_K_ATTN, flops, bytes);
  return a->dtype == CRG_F32 ? dispatch_attn_frames<float>(ctx, st, *a) : dispatch_attn_frames<bf16>(ctx, st, *a);
}

extern "C" int crg_add_frames(crg_ctx* ctx, void* stream, const void* x, const void* e, void* y, int64_t frames, int S, int C, int dtype) {
  if (!ctx) return -22;
  CRG_REQUIRE(ctx, x && e && y && frames >= 1 && S >= 1 && C >= 8 && C % 8 == 0, "add_frames: bad arguments (frames=%lld S=%d C=%d, C %% 8 == 0)",
              (long long)frames, S, C);
  CRG_REQUIRE(ctx, (((uintptr_t)x | (uintptr_t)e | (uintptr_t)y) & 15) == 0, "add_frames: operands must be 16-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  const long n8 = (long)frames * S * (C / 8);
  CRG_REQUIRE(ctx, (n8 + 255) / 256 < (1L << 31), "add_frames: too large");
  crg_prof_scope ps(ctx, st, CRG_K_ELEMENTWISE, 8.0 * n8, 16.0 * n8 * crg_dtype_size(dtype));
  if (dtype == CRG_F32)
    hipLaunchKernelGGL(add_frames_kernel<float>, dim3(ew_grid(n8)), dim3(256), 0, st, (const float*)x, (const float*)e, (float*)y, n8, C / 8, S);
  else if (dtype == CRG_BF16)
    hipLaunchKernelGGL(add_frames_kernel<bf16>, dim3(ew_grid(n8)), dim3(256), 0, st, (const bf16*)x, (const bf16*)e, (bf16*)y, n8, C / 8, S);
  else
    return crg_fail(ctx, -22, "add_frames: dtype %d unsupported", dtype);
  CRG_CHECK_LAUNCH(ctx, "add_frames");
  return 0;
}

extern "C" int crg_lincomb_frames(crg_ctx* ctx, void* stream, const float* a, const void* x, const float* c, const void* z, void* y, int64_t frames,
                                  int64_t per_frame, int dtype) {
  if (!ctx) return -22;
  CRG_REQUIRE(ctx, x && z && y && frames >= 1 && per_frame >= 8 && per_frame % 8 == 0,
              "lincomb_frames: bad arguments (frames=%lld, per_frame=%lld, per_frame %% 8 == 0)", (long long)frames, (long long)per_frame);
  CRG_REQUIRE(ctx, (((uintptr_t)x | (uintptr_t)z | (uintptr_t)y) & 15) == 0, "lincomb_frames: operands must be 16-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  const long n8 = (long)frames * (per_frame / 8);
  CRG_REQUIRE(ctx, (n8 + 255) / 256 < (1L << 31), "lincomb_frames: too large");
  crg_prof_scope ps(ctx, st, CRG_K_ELEMENTWISE, 24.0 * n8, 24.0 * n8 * crg_dtype_size(dtype));
  if (dtype == CRG_F32)
    hipLaunchKernelGGL(lincomb_frames_kernel<float>, dim3(ew_grid(n8)), dim3(256), 0, st, a, (const float*)x, c, (const float*)z, (float*)y, n8, per_frame / 8);
  else if (dtype == CRG_BF16)
    hipLaunchKernelGGL(lincomb_frames_kernel<bf16>, dim3(ew_grid(n8)), dim3(256), 0, st, a, (const bf16*)x, c, (const bf16*)z, (bf16*)y, n8, per_frame / 8);
  else
    return crg_fail(ctx, -22, "lincomb_frames: dtype %d unsupported", dtype);
  CRG_CHECK_LAUNCH(ctx, "lincomb_frames");
  return 0;
}
