// Small / HBM-bound helpers: thin-channel 3x3 conv (conv_in / conv_out), timestep embedding, SiLU,
// NCHW<->NHWC boundary transposes with dtype conversion, affine+clamp cast.
#include "crg_common.h"

namespace {

template <typename T>
__device__ __forceinline__ float ldf(const T* p) { return (float)*p; }

// ---- conv (3x3 or 1x1), Cin <= 8 (conv_in): thread = (PX consecutive pixels of one image row, 8 output channels); weights in
// LDS as [tap*Cin + ci][Cout] fp32; the 8 outputs are one 16-byte store.  Round 3: the kernel size is a template parameter (the
// runtime tap / ks, tap % ks and the 64-bit index divisions were more instructions than the FMAs), the weight image is filled by a
// coalesced linear read, the PX + 2 input pixels of a kernel row are loaded once and shared by its three taps, and the FMAs are packed
// pairs (v_pk_fma_f32): conv_in 4 -> 320 at 8 x 64 x 64 57 -> see DESIGN us.  Widths that are not a multiple of 4 run PX = 1.
template <typename XT, typename YT, int CI, int PX, int KS>
__global__ __launch_bounds__(256) void conv_small_cin_kernel(const XT* __restrict__ x, const float* __restrict__ w,
                                                             const float* __restrict__ bias, YT* __restrict__ y, int N, int H, int W,
                                                             int Cout) {
  extern __shared__ __attribute__((aligned(16))) float wl[];  // [KS*KS*CI][Cout]
  constexpr int taps = KS * KS, pad = KS / 2;
  // weight image: the source [Cout][CI][taps] is read LINEARLY (coalesced) and scattered into LDS
  for (int i = threadIdx.x; i < taps * CI * Cout; i += 256) {
    const int co = i / (taps * CI), r = i - co * (taps * CI);
    const int ci = r / taps, tap = r - ci * taps;
    wl[(tap * CI + ci) * Cout + co] = w[i];
  }
  __syncthreads();
  const int cg = Cout >> 3;  // 8-channel groups
  const int WQ = W / PX;
  const int total = N * H * WQ * cg;  // < 2^31 (checked by the host)
  constexpr int SEG = PX + KS - 1;    // input pixels of one kernel row
  for (int idx = blockIdx.x * 256 + threadIdx.x; idx < total; idx += gridDim.x * 256) {
    const int g = idx % cg;
    const int pq = idx / cg;
    const int wq = pq % WQ, r2 = pq / WQ;
    const int wo0 = wq * PX;
    const int ho = r2 % H;
    const int n = r2 / H;
    f32x2 acc[PX][4];
    {
      f32x4 b0 = {0.f, 0.f, 0.f, 0.f}, b1 = b0;
      if (bias) {
        b0 = *reinterpret_cast<const f32x4*>(bias + g * 8);
        b1 = *reinterpret_cast<const f32x4*>(bias + g * 8 + 4);
      }
#pragma unroll
      for (int px = 0; px < PX; ++px) {
        acc[px][0] = f32x2{b0[0], b0[1]}; acc[px][1] = f32x2{b0[2], b0[3]};
        acc[px][2] = f32x2{b1[0], b1[1]}; acc[px][3] = f32x2{b1[2], b1[3]};
      }
    }
#pragma unroll
    for (int kh = 0; kh < KS; ++kh) {
      const int hi = ho + kh - pad;
      if ((unsigned)hi >= (unsigned)H) continue;
      float xr[SEG][CI];
      const XT* xrow = x + ((long)n * H + hi) * W * CI;
#pragma unroll
      for (int sx = 0; sx < SEG; ++sx) {
        const int wi = wo0 + sx - pad;
        const bool ok = (unsigned)wi < (unsigned)W;
        const XT* xp = xrow + (ok ? wi : 0) * CI;
        if constexpr (CI == 4 && sizeof(XT) == 2) {
          const bf16x4 v = *reinterpret_cast<const bf16x4*>(xp);
#pragma unroll
          for (int c = 0; c < 4; ++c) xr[sx][c] = ok ? (float)v[c] : 0.f;
        } else if constexpr (CI == 4 && sizeof(XT) == 4) {
          const f32x4 v = *reinterpret_cast<const f32x4*>(xp);
#pragma unroll
          for (int c = 0; c < 4; ++c) xr[sx][c] = ok ? v[c] : 0.f;
        } else {
#pragma unroll
          for (int c = 0; c < CI; ++c) xr[sx][c] = ok ? (float)xp[c] : 0.f;
        }
      }
#pragma unroll
      for (int kw = 0; kw < KS; ++kw) {
#pragma unroll
        for (int ci = 0; ci < CI; ++ci) {
          const float* wp = wl + ((kh * KS + kw) * CI + ci) * Cout + g * 8;
          const f32x4 w0 = *reinterpret_cast<const f32x4*>(wp), w1 = *reinterpret_cast<const f32x4*>(wp + 4);
          const f32x2 wa = {w0[0], w0[1]}, wb = {w0[2], w0[3]}, wc = {w1[0], w1[1]}, wd = {w1[2], w1[3]};
#pragma unroll
          for (int px = 0; px < PX; ++px) {
            const float xv = xr[px + kw][ci];
            const f32x2 xx = {xv, xv};
            acc[px][0] = __builtin_elementwise_fma(xx, wa, acc[px][0]);
            acc[px][1] = __builtin_elementwise_fma(xx, wb, acc[px][1]);
            acc[px][2] = __builtin_elementwise_fma(xx, wc, acc[px][2]);
            acc[px][3] = __builtin_elementwise_fma(xx, wd, acc[px][3]);
          }
        }
      }
    }
#pragma unroll
    for (int px = 0; px < PX; ++px) {
      crg_vec8<YT> o;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        o.set(2 * q, acc[px][q][0]);
        o.set(2 * q + 1, acc[px][q][1]);
      }
      o.store(y + (((long)n * H + ho) * W + wo0 + px) * Cout + g * 8);
    }
  }
}

// ---- conv (3x3 or 1x1), Cout <= 8 (conv_out): LPP lanes share one output pixel, each lane walks every LPP-th
// 8-channel chunk of Cin (consecutive lanes -> consecutive 16-byte chunks: coalesced rows), partial sums are
// combined with a shuffle tree.  Weights in LDS as [tap][Cin][CO] fp32, CO = 4 or 8 (the VAE's 3 output channels used to pay for 8),
// compile-time kernel size, packed FMAs.
template <typename XT, typename YT, int CO, int LPP, int KS>
__global__ __launch_bounds__(256) void conv_small_cout_kernel(const XT* __restrict__ x, const float* __restrict__ w,
                                                              const float* __restrict__ bias, YT* __restrict__ y, int N, int H, int W,
                                                              int Cin, int Cout) {
  extern __shared__ __attribute__((aligned(16))) float wl[];  // [KS*KS][Cin][CO]
  constexpr int taps = KS * KS, pad = KS / 2;
  // weight image: zero-fill, then the source [Cout][Cin][taps] read linearly and scattered (see conv_small_cin_kernel)
  for (int i = threadIdx.x; i < taps * Cin * CO; i += 256) wl[i] = 0.f;
  __syncthreads();
  {
    const int per_co = Cin * taps;
    for (int i = threadIdx.x; i < Cout * per_co; i += 256) {
      const int co = i / per_co, r = i - co * per_co;
      const int ci = r / taps, tap = r - ci * taps;
      wl[(tap * Cin + ci) * CO + co] = w[i];
    }
  }
  __syncthreads();
  const int total = N * H * W;  // < 2^31 (checked by the host)
  const int sub = threadIdx.x % LPP;
  constexpr int ppb = 256 / LPP;  // pixels per block iteration
  for (int pix0 = blockIdx.x * ppb; pix0 < total; pix0 += gridDim.x * ppb) {
    const int pix = pix0 + threadIdx.x / LPP;
    const bool live = pix < total;
    const int pp = live ? pix : total - 1;
    const int wo = pp % W, r2 = pp / W;
    const int ho = r2 % H;
    const int n = r2 / H;
    f32x2 acc[CO / 2];
#pragma unroll
    for (int e = 0; e < CO / 2; ++e) acc[e] = f32x2{0.f, 0.f};
#pragma unroll
    for (int tap = 0; tap < taps; ++tap) {
      const int hi = ho + tap / KS - pad, wi = wo + tap % KS - pad;
      if ((unsigned)hi >= (unsigned)H || (unsigned)wi >= (unsigned)W) continue;
      const XT* xp = x + (((long)n * H + hi) * W + wi) * Cin;
      const float* wt = wl + tap * Cin * CO;
      if ((Cin & 7) == 0) {
        for (int c0 = sub * 8; c0 < Cin; c0 += LPP * 8) {
          crg_vec8<XT> v;
          v.load(xp + c0);
#pragma unroll
          for (int j = 0; j < 8; ++j) {
            const float xv = v.get(j);
            const f32x2 xx = {xv, xv};
            const float* wp = wt + (c0 + j) * CO;
#pragma unroll
            for (int e = 0; e < CO / 2; ++e) acc[e] = __builtin_elementwise_fma(xx, *reinterpret_cast<const f32x2*>(wp + 2 * e), acc[e]);
          }
        }
      } else {
        for (int ci = sub; ci < Cin; ci += LPP) {
          const float xv = ldf(xp + ci);
          const f32x2 xx = {xv, xv};
#pragma unroll
          for (int e = 0; e < CO / 2; ++e) acc[e] = __builtin_elementwise_fma(xx, *reinterpret_cast<const f32x2*>(wt + ci * CO + 2 * e), acc[e]);
        }
      }
    }
#pragma unroll
    for (int o = 1; o < LPP; o <<= 1)
#pragma unroll
      for (int e = 0; e < CO / 2; ++e) {
        acc[e][0] += __shfl_xor(acc[e][0], o);
        acc[e][1] += __shfl_xor(acc[e][1], o);
      }
    if (live && sub == 0) {
      YT* yp = y + (long)pix * Cout;
#pragma unroll
      for (int e = 0; e < CO; ++e)
        if (e < Cout) yp[e] = (YT)(acc[e >> 1][e & 1] + (bias ? bias[e] : 0.f));
    }
  }
}

template <typename YT>
__global__ void timestep_embedding_kernel(const float* __restrict__ t, YT* __restrict__ out, int B, int dim) {
  const int half = dim / 2;
  const int idx = blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= B * dim) return;
  const int b = idx / dim, j = idx - b * dim;
  float v = 0.f;
  if (j < 2 * half) {
    const int i = j < half ? j : j - half;
    // freqs = exp(-ln(10000) * i / half) in fp32, as util.py:162-164 builds them
    const float f = expf(-9.210340371976184f * (float)i / (float)half);
    const float a = t[b] * f;
    v = j < half ? cosf(a) : sinf(a);
  }
  out[idx] = (YT)v;
}

template <typename T>
__global__ void silu_kernel(const T* __restrict__ x, T* __restrict__ y, long n) {
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x)
    y[i] = (T)crg_silu_f((float)x[i]);
}

// NCHW -> NHWC via a 32x32 LDS tile transpose: src [N][C][HW], dst [N][HW][C]
template <typename ST, typename DT>
__global__ __launch_bounds__(256) void transpose_kernel(const ST* __restrict__ src, DT* __restrict__ dst, int R, int Cc) {
  // src viewed as [N][R][Cc], dst as [N][Cc][R]
  __shared__ float tile[32][33];
  const int n = blockIdx.z;
  const int r0 = blockIdx.y * 32, c0 = blockIdx.x * 32;
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;  // 32 x 8
  const ST* s = src + (long)n * R * Cc;
  DT* d = dst + (long)n * R * Cc;
  for (int i = ty; i < 32; i += 8) {
    const int rr = r0 + i, cc = c0 + tx;
    tile[i][tx] = (rr < R && cc < Cc) ? (float)s[(long)rr * Cc + cc] : 0.f;
  }
  __syncthreads();
  for (int i = ty; i < 32; i += 8) {
    const int cc = c0 + i, rr = r0 + tx;
    if (rr < R && cc < Cc) d[(long)cc * R + rr] = (DT)tile[tx][i];
  }
}

// cat([a, b], dim 1) of two NCHW tensors -> one NHWC tensor, the concat folded into the transpose: a [N][Ca][HW], b [N][Cb][HW],
// dst [N][HW][Ca + Cb].  Channel rows below Ca come from a, the rest from b (same 32x32 tile walk as transpose_kernel).
template <typename ST, typename DT>
__global__ __launch_bounds__(256) void transpose_cat_kernel(const ST* __restrict__ a, const ST* __restrict__ b, DT* __restrict__ dst, int Ca,
                                                            int Cb, int HW) {
  __shared__ float tile[32][33];
  const int n = blockIdx.z;
  const int C = Ca + Cb;
  const int r0 = blockIdx.y * 32, c0 = blockIdx.x * 32;  // r: channel, c: pixel
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  const ST* sa = a + (long)n * Ca * HW;
  const ST* sb = b + (long)n * Cb * HW;
  DT* d = dst + (long)n * C * HW;
  for (int i = ty; i < 32; i += 8) {
    const int rr = r0 + i, cc = c0 + tx;
    float v = 0.f;
    if (rr < C && cc < HW) v = rr < Ca ? (float)sa[(long)rr * HW + cc] : (float)sb[(long)(rr - Ca) * HW + cc];
    tile[i][tx] = v;
  }
  __syncthreads();
  for (int i = ty; i < 32; i += 8) {
    const int cc = c0 + i, rr = r0 + tx;
    if (rr < C && cc < HW) d[(long)cc * C + rr] = (DT)tile[tx][i];
  }
}

template <typename ST, typename DT>
__global__ void affine_cast_kernel(const ST* __restrict__ x, DT* __restrict__ y, long n, float a, float b, float lo, float hi) {
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
    float v = (float)x[i] * a + b;
    v = fminf(fmaxf(v, lo), hi);
    y[i] = (DT)v;
  }
}

template <typename T>
__global__ void axpby_kernel(const T* __restrict__ x, T* __restrict__ y, long n, float a, float b) {
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x)
    y[i] = (T)(a * (float)x[i] + b * (float)y[i]);
}

template <typename F>
int by_dtype2(crg_ctx* ctx, int sdt, int ddt, const char* what, F&& f) {
  if (sdt == CRG_BF16 && ddt == CRG_BF16) return f((const bf16*)nullptr, (bf16*)nullptr);
  if (sdt == CRG_BF16 && ddt == CRG_F32) return f((const bf16*)nullptr, (float*)nullptr);
  if (sdt == CRG_F32 && ddt == CRG_BF16) return f((const float*)nullptr, (bf16*)nullptr);
  if (sdt == CRG_F32 && ddt == CRG_F32) return f((const float*)nullptr, (float*)nullptr);
  return crg_fail(ctx, -22, "%s: unsupported dtype pair %d -> %d", what, sdt, ddt);
}

inline int grid_for(long n) {
  long g = (n + 255) / 256;
  return (int)(g < 1 ? 1 : (g > 8192 ? 8192 : g));
}

// grid for kernels that first stage an `lds`-byte weight image per block: as many blocks as fit the chip at once
// (256 CUs x blocks/CU limited by the 160 KiB LDS), never more than the work needs
inline int grid_resident(long n_threads, size_t lds) {
  long per_cu = lds ? (long)((160 * 1024) / lds) : 8;
  if (per_cu < 1) per_cu = 1;
  if (per_cu > 8) per_cu = 8;
  long g = (n_threads + 255) / 256;
  const long cap = 256 * per_cu;
  return (int)(g < 1 ? 1 : (g > cap ? cap : g));
}

}  // namespace

extern "C" int crg_conv_small(crg_ctx* ctx, void* stream, const void* x, const float* w, const float* bias, void* y,
                              int N, int H, int W, int Cin, int Cout, int ksize, int x_dtype, int y_dtype) {
  if (!ctx) return -22;
  CRG_REQUIRE(ctx, N > 0 && H > 0 && W > 0 && Cin > 0 && Cout > 0, "conv_small: empty problem");
  CRG_REQUIRE(ctx, Cin <= 9 || Cout <= 8, "conv_small: needs Cin <= 9 or Cout <= 8 (Cin=%d Cout=%d)", Cin, Cout);
  hipStream_t st = (hipStream_t)stream;
  const int ks = ksize;
  CRG_REQUIRE(ctx, ks == 1 || ks == 3, "conv_small: ksize %d unsupported", ks);
  const double flops = 2.0 * N * H * W * (double)Cin * Cout * ks * ks;
  const double bytes = (double)N * H * W * (Cin * crg_dtype_size(x_dtype) + Cout * crg_dtype_size(y_dtype));
  crg_prof_scope ps(ctx, st, CRG_K_CONV_SMALL, flops, bytes);
  CRG_REQUIRE(ctx, (double)N * H * W * (Cout > 8 ? Cout / 8 : 1) < 2147483648.0, "conv_small: more than 2^31 work items");
  int rc;
  if (Cout <= 8 && (Cin > 8 || Cout <= Cin)) {
    const int CO = Cout <= 4 ? 4 : 8;
    const size_t lds = (size_t)ks * ks * Cin * CO * sizeof(float);
    CRG_REQUIRE(ctx, lds <= 160 * 1024, "conv_small: Cin=%d too large for the LDS weight image", Cin);
    if ((Cin & 7) == 0) CRG_REQUIRE(ctx, ((uintptr_t)x & 15) == 0, "conv_small: x must be 16-byte aligned");
    rc = by_dtype2(ctx, x_dtype, y_dtype, "conv_small", [&](auto* xs, auto* ys) {
      using XT = std::remove_const_t<std::remove_pointer_t<decltype(xs)>>;
      using YT = std::remove_pointer_t<decltype(ys)>;
      const long pixels = (long)N * H * W;
      const bool wide = Cin >= 64;  // eight lanes per pixel
      auto go = [&](auto kern) {
        if (lds > 64 * 1024) (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        hipLaunchKernelGGL(kern, dim3(grid_resident(wide ? pixels * 8 : pixels, lds)), dim3(256), lds, st, (const XT*)x, w, bias, (YT*)y, N, H, W, Cin, Cout);
      };
      if (ks == 3) {
        if (CO == 4) wide ? go(conv_small_cout_kernel<XT, YT, 4, 8, 3>) : go(conv_small_cout_kernel<XT, YT, 4, 1, 3>);
        else wide ? go(conv_small_cout_kernel<XT, YT, 8, 8, 3>) : go(conv_small_cout_kernel<XT, YT, 8, 1, 3>);
      } else {
        if (CO == 4) wide ? go(conv_small_cout_kernel<XT, YT, 4, 8, 1>) : go(conv_small_cout_kernel<XT, YT, 4, 1, 1>);
        else wide ? go(conv_small_cout_kernel<XT, YT, 8, 8, 1>) : go(conv_small_cout_kernel<XT, YT, 8, 1, 1>);
      }
      return 0;
    });
  } else {
    CRG_REQUIRE(ctx, Cout % 8 == 0, "conv_small: Cout=%d must be a multiple of 8 when Cin <= 8", Cout);
    CRG_REQUIRE(ctx, Cin == 3 || Cin == 4 || Cin == 8 || Cin == 9, "conv_small: Cin=%d unsupported on the thin-input path (3, 4, 8 or 9)",
                Cin);
    const size_t lds = (size_t)ks * ks * Cin * Cout * sizeof(float);
    CRG_REQUIRE(ctx, lds <= 160 * 1024, "conv_small: Cout=%d too large for the LDS weight image", Cout);
    rc = by_dtype2(ctx, x_dtype, y_dtype, "conv_small", [&](auto* xs, auto* ys) {
      using XT = std::remove_const_t<std::remove_pointer_t<decltype(xs)>>;
      using YT = std::remove_pointer_t<decltype(ys)>;
      // 4 pixels per thread (8-channel inputs would need 32 more registers: one pixel).  The 9-channel conv_in of the inpainting
      // UNet (4 latent + 1 mask + 4 masked-image channels) keeps a 101 KiB weight image, i.e. one block per CU and one wave per SIMD:
      // there the registers are free and the four pixels' independent FMA chains are the only latency hiding left.
      const bool quad = W % 4 == 0 && (Cin <= 4 || Cin == 9);
      const dim3 grid(grid_resident((long)N * H * (quad ? W / 4 : W) * (Cout / 8), lds));
      auto go = [&](auto kern) {
        if (lds > 64 * 1024) (void)hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        hipLaunchKernelGGL(kern, grid, dim3(256), lds, st, (const XT*)x, w, bias, (YT*)y, N, H, W, Cout);
      };
      if (ks == 3) {
        if (Cin == 3) quad ? go(conv_small_cin_kernel<XT, YT, 3, 4, 3>) : go(conv_small_cin_kernel<XT, YT, 3, 1, 3>);
        else if (Cin == 4) quad ? go(conv_small_cin_kernel<XT, YT, 4, 4, 3>) : go(conv_small_cin_kernel<XT, YT, 4, 1, 3>);
        else if (Cin == 9) quad ? go(conv_small_cin_kernel<XT, YT, 9, 4, 3>) : go(conv_small_cin_kernel<XT, YT, 9, 1, 3>);
        else go(conv_small_cin_kernel<XT, YT, 8, 1, 3>);
      } else {
        if (Cin == 3) quad ? go(conv_small_cin_kernel<XT, YT, 3, 4, 1>) : go(conv_small_cin_kernel<XT, YT, 3, 1, 1>);
        else if (Cin == 4) quad ? go(conv_small_cin_kernel<XT, YT, 4, 4, 1>) : go(conv_small_cin_kernel<XT, YT, 4, 1, 1>);
        else if (Cin == 9) go(conv_small_cin_kernel<XT, YT, 9, 1, 1>);
        else go(conv_small_cin_kernel<XT, YT, 8, 1, 1>);
      }
      return 0;
    });
  }
  if (rc) return rc;
  CRG_CHECK_LAUNCH(ctx, "conv_small");
  return 0;
}

extern "C" int crg_timestep_embedding(crg_ctx* ctx, void* stream, const float* t, void* out, int B, int dim, int dtype) {
  if (!ctx) return -22;
  CRG_REQUIRE(ctx, B > 0 && dim > 0, "timestep_embedding: empty");
  hipStream_t st = (hipStream_t)stream;
  crg_prof_scope ps(ctx, st, CRG_K_ELEMENTWISE, 4.0 * B * dim, (double)B * dim * crg_dtype_size(dtype));
  const int n = B * dim;
  if (dtype == CRG_F32)
    hipLaunchKernelGGL(timestep_embedding_kernel<float>, dim3((n + 255) / 256), dim3(256), 0, st, t, (float*)out, B, dim);
  else if (dtype == CRG_BF16)
    hipLaunchKernelGGL(timestep_embedding_kernel<bf16>, dim3((n + 255) / 256), dim3(256), 0, st, t, (bf16*)out, B, dim);
  else
    return crg_fail(ctx, -22, "timestep_embedding: dtype %d unsupported", dtype);
  CRG_CHECK_LAUNCH(ctx, "timestep_embedding");
  return 0;
}

extern "C" int crg_silu(crg_ctx* ctx, void* stream, const void* x, void* y, int64_t n, int dtype) {
  if (!ctx) return -22;
  CRG_REQUIRE(ctx, n > 0, "silu: empty");
  hipStream_t st = (hipStream_t)stream;
  crg_prof_scope ps(ctx, st, CRG_K_ELEMENTWISE, 4.0 * n, 2.0 * n * crg_dtype_size(dtype));
  if (dtype == CRG_F32)
    hipLaunchKernelGGL(silu_kernel<float>, dim3(grid_for(n)), dim3(256), 0, st, (const float*)x, (float*)y, (long)n);
  else if (dtype == CRG_BF16)
    hipLaunchKernelGGL(silu_kernel<bf16>, dim3(grid_for(n)), dim3(256), 0, st, (const bf16*)x, (bf16*)y, (long)n);
  else
    return crg_fail(ctx, -22, "silu: dtype %d unsupported", dtype);
  CRG_CHECK_LAUNCH(ctx, "silu");
  return 0;
}

static int transpose_impl(crg_ctx* ctx, void* stream, const void* src, void* dst, int N, int R, int Cc, int sdt, int ddt,
                          const char* what) {
  CRG_REQUIRE(ctx, N > 0 && R > 0 && Cc > 0, "%s: empty", what);
  hipStream_t st = (hipStream_t)stream;
  const double elems = (double)N * R * Cc;
  crg_prof_scope ps(ctx, st, CRG_K_ELEMENTWISE, 0.0, elems * (crg_dtype_size(sdt) + crg_dtype_size(ddt)));
  dim3 grid((Cc + 31) / 32, (R + 31) / 32, N);
  int rc = by_dtype2(ctx, sdt, ddt, what, [&](auto* xs, auto* ys) {
    using ST = std::remove_const_t<std::remove_pointer_t<decltype(xs)>>;
    using DT = std::remove_pointer_t<decltype(ys)>;
    hipLaunchKernelGGL((transpose_kernel<ST, DT>), grid, dim3(256), 0, st, (const ST*)src, (DT*)dst, R, Cc);
    return 0;
  });
  if (rc) return rc;
  CRG_CHECK_LAUNCH(ctx, what);
  return 0;
}

extern "C" int crg_nchw_to_nhwc(crg_ctx* ctx, void* stream, const void* src, void* dst, int N, int C, int HW, int src_dtype,
                                int dst_dtype) {
  if (!ctx) return -22;
  return transpose_impl(ctx, stream, src, dst, N, C, HW, src_dtype, dst_dtype, "nchw_to_nhwc");
}

extern "C" int crg_nhwc_to_nchw(crg_ctx* ctx, void* stream, const void* src, void* dst, int N, int C, int HW, int src_dtype,
                                int dst_dtype) {
  if (!ctx) return -22;
  return transpose_impl(ctx, stream, src, dst, N, HW, C, src_dtype, dst_dtype, "nhwc_to_nchw");
}

extern "C" int crg_nchw2_to_nhwc(crg_ctx* ctx, void* stream, const void* src_a, const void* src_b, void* dst, int N, int Ca, int Cb,
                                 int HW, int src_dtype, int dst_dtype) {
  if (!ctx) return -22;
  CRG_REQUIRE(ctx, N > 0 && Ca > 0 && Cb > 0 && HW > 0 && src_a && src_b && dst, "nchw2_to_nhwc: empty");
  hipStream_t st = (hipStream_t)stream;
  const double elems = (double)N * (Ca + Cb) * HW;
  crg_prof_scope ps(ctx, st, CRG_K_ELEMENTWISE, 0.0, elems * (crg_dtype_size(src_dtype) + crg_dtype_size(dst_dtype)));
  dim3 grid((HW + 31) / 32, (Ca + Cb + 31) / 32, N);
  int rc = by_dtype2(ctx, src_dtype, dst_dtype, "nchw2_to_nhwc", [&](auto* xs, auto* ys) {
    using ST = std::remove_const_t<std::remove_pointer_t<decltype(xs)>>;
    using DT = std::remove_pointer_t<decltype(ys)>;
    hipLaunchKernelGGL((transpose_cat_kernel<ST, DT>), grid, dim3(256), 0, st, (const ST*)src_a, (const ST*)src_b, (DT*)dst, Ca, Cb, HW);
    return 0;
  });
  if (rc) return rc;
  CRG_CHECK_LAUNCH(ctx, "nchw2_to_nhwc");
  return 0;
}

extern "C" int crg_affine_cast(crg_ctx* ctx, void* stream, const void* x, void* y, int64_t n, float a, float b, float lo,
                               float hi, int src_dtype, int dst_dtype) {
  if (!ctx) return -22;
  CRG_REQUIRE(ctx, n > 0, "affine_cast: empty");
  hipStream_t st = (hipStream_t)stream;
  crg_prof_scope ps(ctx, st, CRG_K_ELEMENTWISE, 2.0 * n, (double)n * (crg_dtype_size(src_dtype) + crg_dtype_size(dst_dtype)));
  int rc = by_dtype2(ctx, src_dtype, dst_dtype, "affine_cast", [&](auto* xs, auto* ys) {
    using ST = std::remove_const_t<std::remove_pointer_t<decltype(xs)>>;
    using DT = std::remove_pointer_t<decltype(ys)>;
    hipLaunchKernelGGL((affine_cast_kernel<ST, DT>), dim3(grid_for(n)), dim3(256), 0, st, (const ST*)x, (DT*)y, (long)n, a, b, lo, hi);
    return 0;
  });
  if (rc) return rc;
  CRG_CHECK_LAUNCH(ctx, "affine_cast");
  return 0;
}

namespace {
__global__ __launch_bounds__(256) void split_bf16_kernel(const float* __restrict__ x, bf16* __restrict__ hi, bf16* __restrict__ lo, long n8) {
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n8; i += (long)gridDim.x * 256) {
    const f32x4 a = *reinterpret_cast<const f32x4*>(x + i * 8), b = *reinterpret_cast<const f32x4*>(x + i * 8 + 4);
    bf16x8 h8, l8;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const float f = e < 4 ? a[e] : b[e - 4];
      const bf16 h = (bf16)f;
      h8[e] = h;
      l8[e] = (bf16)(f - (float)h);
    }
    *reinterpret_cast<bf16x8*>(hi + i * 8) = h8;
    *reinterpret_cast<bf16x8*>(lo + i * 8) = l8;
  }
}
}  // namespace

namespace {
// fp32 [pixels][C] -> MX planes (CRG_PREC_F16MX): thread = eight channels of one pixel
__global__ __launch_bounds__(256) void split_mx_kernel(const float* __restrict__ x, _Float16* __restrict__ x16, unsigned char* __restrict__ x8,
                                                       long n8, int C, float sh, float sl) {
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n8; i += (long)gridDim.x * 256) {
    const long e = i * 8;  // element index = pixel * C + c0
    const int c0 = (int)(e % C);
    const f32x4 a = *reinterpret_cast<const f32x4*>(x + e), b = *reinterpret_cast<const f32x4*>(x + e + 4);
    const float f[8] = {a[0], a[1], a[2], a[3], b[0], b[1], b[2], b[3]};
    crg_store_mx8(f, x16 + e, x8 + 2 * (e - (c0 & 63)) + (c0 & 63), sh, sl);
  }
}
}  // namespace

extern "C" int crg_split_mx(crg_ctx* ctx, void* stream, const void* x, void* x16, void* x8, int64_t pixels, int C, int hi_log2, int lo_log2) {
  if (!ctx) return -22;
  CRG_REQUIRE(ctx, pixels > 0 && C > 0 && C % 64 == 0, "split_mx: C=%d must be a positive multiple of 64", C);
  CRG_REQUIRE(ctx, (((uintptr_t)x | (uintptr_t)x16 | (uintptr_t)x8) & 15) == 0, "split_mx: pointers must be 16-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  const long n = (long)pixels * C;
  crg_prof_scope ps(ctx, st, CRG_K_ELEMENTWISE, 6.0 * n, 8.0 * n);
  hipLaunchKernelGGL(split_mx_kernel, dim3(grid_for(n / 8)), dim3(256), 0, st, (const float*)x, (_Float16*)x16, (unsigned char*)x8, n / 8, C,
                     ldexpf(1.f, hi_log2), ldexpf(1.f, lo_log2));
  CRG_CHECK_LAUNCH(ctx, "split_mx");
  return 0;
}

extern "C" int crg_split_bf16(crg_ctx* ctx, void* stream, const void* x, void* hi, void* lo, int64_t n) {
  if (!ctx) return -22;
  CRG_REQUIRE(ctx, n > 0 && n % 8 == 0, "split_bf16: element count %ld must be a positive multiple of 8", (long)n);
  CRG_REQUIRE(ctx, (((uintptr_t)x | (uintptr_t)hi | (uintptr_t)lo) & 15) == 0, "split_bf16: pointers must be 16-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  crg_prof_scope ps(ctx, st, CRG_K_ELEMENTWISE, 3.0 * n, 8.0 * n);
  hipLaunchKernelGGL(split_bf16_kernel, dim3(grid_for(n / 8)), dim3(256), 0, st, (const float*)x, (bf16*)hi, (bf16*)lo, (long)(n / 8));
  CRG_CHECK_LAUNCH(ctx, "split_bf16");
  return 0;
}

namespace {
// One fused sampler step (see include/crg_hip.h); the arithmetic follows the reference's operation order one rounding at a
// time (no FMA contraction), so the result equals the chain of PyTorch elementwise kernels it replaces.
__global__ __launch_bounds__(256) void cfg_euler_step_kernel(float* __restrict__ x, const float* __restrict__ eps,
                                                             const float* __restrict__ noise, long n, float sigma, float dt,
                                                             float cfg, float noise_scale) {
#pragma clang fp contract(off)
  const float c_out = -sigma;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
    const float xv = x[i];
    const float den_u = xv + eps[i] * c_out;
    const float den_c = xv + eps[n + i] * c_out;
    const float den = den_u + cfg * (den_c - den_u);
    const float d = (xv - den) / sigma;
    float xn = xv + d * dt;
    if (noise) xn = xn + noise[i] * noise_scale;
    x[i] = xn;
  }
}
}  // namespace

extern "C" int crg_cfg_euler_step(crg_ctx* ctx, void* stream, void* x, const void* eps, const void* noise, int64_t n, float sigma,
                                  float dt, float cfg_scale, float noise_scale) {
  if (!ctx) return -22;
  CRG_REQUIRE(ctx, n > 0 && x && eps, "cfg_euler_step: empty input");
  CRG_REQUIRE(ctx, sigma > 0.f, "cfg_euler_step: sigma must be positive (got %g)", (double)sigma);
  hipStream_t st = (hipStream_t)stream;
  crg_prof_scope ps(ctx, st, CRG_K_ELEMENTWISE, 10.0 * n, 4.0 * n * (noise ? 5 : 4));
  hipLaunchKernelGGL(cfg_euler_step_kernel, dim3(grid_for(n)), dim3(256), 0, st, (float*)x, (const float*)eps, (const float*)noise, (long)n,
                     sigma, dt, cfg_scale, noise_scale);
  CRG_CHECK_LAUNCH(ctx, "cfg_euler_step");
  return 0;
}

namespace {
// One fused DDIM step (see include/crg_hip.h): p_sample_ddim's elementwise chain, one fp32 rounding per operation in the reference's
// order (no FMA contraction).  The per-step scalars arrive already rounded to fp32, as torch.full((b,1,1,1), table[index]) does.
__global__ __launch_bounds__(256) void cfg_ddim_step_kernel(float* __restrict__ x, const float* __restrict__ eps,
                                                            const float* __restrict__ noise, long n, float cfg, float sqrt_one_minus_a,
                                                            float sqrt_a, float sqrt_a_prev, float dir_coef, float sigma) {
#pragma clang fp contract(off)
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
    const float eu = eps[i];
    const float e = eu + cfg * (eps[n + i] - eu);
    const float xv = x[i];
    const float x0 = (xv - sqrt_one_minus_a * e) / sqrt_a;
    const float dir = dir_coef * e;
    float xn = sqrt_a_prev * x0 + dir;
    if (noise) xn = xn + sigma * noise[i];
    x[i] = xn;
  }
}
}  // namespace

extern "C" int crg_cfg_ddim_step(crg_ctx* ctx, void* stream, void* x, const void* eps, const void* noise, int64_t n, float cfg_scale,
                                 float sqrt_one_minus_a, float sqrt_a, float sqrt_a_prev, float dir_coef, float sigma) {
  if (!ctx) return -22;
  CRG_REQUIRE(ctx, n > 0 && x && eps, "cfg_ddim_step: empty input");
  CRG_REQUIRE(ctx, sqrt_a > 0.f, "cfg_ddim_step: sqrt(alpha) must be positive (got %g)", (double)sqrt_a);
  CRG_REQUIRE(ctx, sigma == 0.f || noise, "cfg_ddim_step: sigma %g > 0 needs a noise tensor", (double)sigma);
  hipStream_t st = (hipStream_t)stream;
  if (sigma == 0.f) noise = nullptr;  // eta = 0: the noise term is sigma * z = 0, nothing to read
  crg_prof_scope ps(ctx, st, CRG_K_ELEMENTWISE, 10.0 * n, 4.0 * n * (noise ? 5 : 4));
  hipLaunchKernelGGL(cfg_ddim_step_kernel, dim3(grid_for(n)), dim3(256), 0, st, (float*)x, (const float*)eps, (const float*)noise, (long)n,
                     cfg_scale, sqrt_one_minus_a, sqrt_a, sqrt_a_prev, dir_coef, sigma);
  CRG_CHECK_LAUNCH(ctx, "cfg_ddim_step");
  return 0;
}

namespace {
// One fused DPM++ 2M step (see include/crg_hip.h): DiscreteDenoiser (EpsScaling, c_skip = 1) on both CFG halves, VanillaCFG and
// DPMPP2MSampler.sampler_step's update, one fp32 rounding per operation in the reference's order (no FMA contraction).  `old` is
// read only on an advanced step, so the first step may pass an uninitialised buffer; it always receives this step's denoised value.
__global__ __launch_bounds__(256) void cfg_dpmpp2m_step_kernel(float* __restrict__ x, const float* __restrict__ eps,
                                                               float* __restrict__ old, long n, float c_out, float cfg, float m1,
                                                               float m2, float m3, float m4, int advanced) {
#pragma clang fp contract(off)
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
    const float xv = x[i];
    const float den_u = eps[i] * c_out + xv;
    const float den_c = eps[n + i] * c_out + xv;
    const float den = den_u + cfg * (den_c - den_u);
    float xn;
    if (advanced) {
      const float dd = m3 * den - m4 * old[i];
      xn = m1 * xv - m2 * dd;
    } else {
      xn = m1 * xv - m2 * den;
    }
    x[i] = xn;
    old[i] = den;
  }
}
}  // namespace

extern "C" int crg_cfg_dpmpp2m_step(crg_ctx* ctx, void* stream, void* x, const void* eps, void* old_den, int64_t n, float c_out,
                                    float cfg_scale, float m1, float m2, float m3, float m4, int advanced) {
  if (!ctx) return -22;
  CRG_REQUIRE(ctx, n > 0 && x && eps && old_den, "cfg_dpmpp2m_step: empty input");
  hipStream_t st = (hipStream_t)stream;
  crg_prof_scope ps(ctx, st, CRG_K_ELEMENTWISE, (advanced ? 11.0 : 8.0) * n, 4.0 * n * (advanced ? 6 : 5));
  hipLaunchKernelGGL(cfg_dpmpp2m_step_kernel, dim3(grid_for(n)), dim3(256), 0, st, (float*)x, (const float*)eps, (float*)old_den,
                     (long)n, c_out, cfg_scale, m1, m2, m3, m4, advanced ? 1 : 0);
  CRG_CHECK_LAUNCH(ctx, "cfg_dpmpp2m_step");
  return 0;
}

namespace {
// One fused k-sampler evaluation step (see include/crg_hip.h, crg_sampler_step_args): the denoiser scalings and the guidance of the
// evaluation's input xin, then the kind's update, one fp32 rounding per operation in the reference's order (no FMA contraction).
// The arguments travel by value (kernel arguments); a buffer the kind does not use on this step is never dereferenced.
__global__ __launch_bounds__(256) void cfg_sampler_step_kernel(crg_sampler_step_args a) {
#pragma clang fp contract(off)
  const long n = (long)a.n;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
    const bool second = a.kind == CRG_STEP_HEUN_2 || a.kind == CRG_STEP_DPMPP2S_2;
    const float xv = a.x[i];
    const float xin = second ? a.x2[i] : xv;
    const float den_u = a.eps[i] * a.c_out + xin;
    const float den_c = a.eps[n + i] * a.c_out + xin;
    const float den = den_u + a.cfg_scale * (den_c - den_u);
    float xn = xv;
    bool noised = false, store_x = true;
    switch (a.kind) {
      case CRG_STEP_HEUN_1: {
        const float d = (xv - den) / a.sigma;
        const float x2 = xv + a.dt * d;
        if (a.one_call) {
          xn = x2;
        } else {
          a.x2[i] = x2;
          a.d[i] = d;
          store_x = false;
        }
        break;
      }
      case CRG_STEP_HEUN_2: {
        const float d2 = (xin - den) / a.sigma;
        const float dp = (a.d[i] + d2) / 2.0f;
        xn = xv + dp * a.dt;
        break;
      }
      case CRG_STEP_DPMPP2S_1:
        if (!a.one_call) {
          a.x2[i] = a.m[0] * xv - a.m[1] * den;
          store_x = false;
          break;
        }
        [[fallthrough]];
      case CRG_STEP_EULER_A: {
        const float d = (xv - den) / a.sigma;
        xn = xv + a.dt * d;
        noised = true;
        break;
      }
      case CRG_STEP_DPMPP2S_2:
        xn = a.m[2] * xv - a.m[3] * den;
        noised = true;
        break;
      case CRG_STEP_LMS: {
        const float d = (xv - den) / a.sigma;
        a.d[i] = d;
        float acc = a.coef[0] * d;
        for (int k = 0; k < a.n_hist; ++k) acc = acc + a.coef[k + 1] * a.hist[k][i];
        xn = xv + acc;
        break;
      }
      default:
        break;
    }
    if (noised && a.add_noise) xn = xn + (a.noise[i] * a.s_noise) * a.sigma_up;
    if (store_x) a.x[i] = xn;
  }
}
}  // namespace

extern "C" int crg_cfg_sampler_step(crg_ctx* ctx, void* stream, const crg_sampler_step_args* args) {
  if (!ctx) return -22;
  CRG_REQUIRE(ctx, args != nullptr, "cfg_sampler_step: null args");
  const crg_sampler_step_args& a = *args;
  const int k = a.kind;
  CRG_REQUIRE(ctx, k >= CRG_STEP_EULER_A && k <= CRG_STEP_LMS, "cfg_sampler_step: unknown kind %d", k);
  CRG_REQUIRE(ctx, a.n > 0 && a.x && a.eps, "cfg_sampler_step: empty input");
  const bool two_call_first = (k == CRG_STEP_HEUN_1 || k == CRG_STEP_DPMPP2S_1) && !a.one_call;
  const bool divides = k == CRG_STEP_EULER_A || k == CRG_STEP_HEUN_1 || k == CRG_STEP_HEUN_2 || k == CRG_STEP_LMS ||
                       (k == CRG_STEP_DPMPP2S_1 && a.one_call);
  const bool may_noise = k == CRG_STEP_EULER_A || k == CRG_STEP_DPMPP2S_2 || (k == CRG_STEP_DPMPP2S_1 && a.one_call);
  CRG_REQUIRE(ctx, !divides || a.sigma > 0.f, "cfg_sampler_step: kind %d divides by sigma, which must be positive (got %g)", k,
              (double)a.sigma);
  CRG_REQUIRE(ctx, !(two_call_first || k == CRG_STEP_HEUN_2 || k == CRG_STEP_DPMPP2S_2) || a.x2, "cfg_sampler_step: kind %d needs x2", k);
  CRG_REQUIRE(ctx, !((k == CRG_STEP_HEUN_1 && !a.one_call) || k == CRG_STEP_HEUN_2 || k == CRG_STEP_LMS) || a.d,
              "cfg_sampler_step: kind %d needs d", k);
  CRG_REQUIRE(ctx, !may_noise || !a.add_noise || a.noise, "cfg_sampler_step: add_noise needs a noise tensor");
  if (k == CRG_STEP_LMS) {
    CRG_REQUIRE(ctx, a.n_hist >= 0 && a.n_hist <= 3, "cfg_sampler_step: n_hist %d out of 0..3", a.n_hist);
    for (int h = 0; h < a.n_hist; ++h) CRG_REQUIRE(ctx, a.hist[h] != nullptr, "cfg_sampler_step: hist[%d] is null", h);
  }
  crg_sampler_step_args kargs = a;
  if (!may_noise || !kargs.add_noise) {  // nothing noise-related is read
    kargs.add_noise = 0;
    kargs.noise = nullptr;
  }
  if (k != CRG_STEP_LMS) kargs.n_hist = 0;
  hipStream_t st = (hipStream_t)stream;
  // x, both eps halves and one store, plus what the kind adds
  const double words = 4.0 + (k == CRG_STEP_HEUN_1 && two_call_first ? 1.0 : 0.0) + (k == CRG_STEP_HEUN_2 ? 2.0 : 0.0) +
                       (k == CRG_STEP_DPMPP2S_2 ? 1.0 : 0.0) + (k == CRG_STEP_LMS ? 1.0 + kargs.n_hist : 0.0) + (kargs.add_noise ? 1.0 : 0.0);
  crg_prof_scope ps(ctx, st, CRG_K_ELEMENTWISE, 12.0 * a.n, 4.0 * a.n * words);
  hipLaunchKernelGGL(cfg_sampler_step_kernel, dim3(grid_for(a.n)), dim3(256), 0, st, kargs);
  CRG_CHECK_LAUNCH(ctx, "cfg_sampler_step");
  return 0;
}

namespace {
// One fused evaluation step of the SD1.5 k-diffusion samplers cfg_sampler_step_kernel does not cover (see include/crg_hip.h,
// crg_kstep_args): the same denoiser scalings and guidance, then the kind's update, one fp32 rounding per operation in the
// reference's order (no FMA contraction).  Arguments by value; a buffer the kind or branch does not use is never dereferenced.
__global__ __launch_bounds__(256) void cfg_kstep_kernel(crg_kstep_args a) {
#pragma clang fp contract(off)
  const long n = (long)a.n;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
    const float xv = a.x[i];
    const float xin = a.kind == CRG_KSTEP_DPM2_2 ? a.x2[i] : xv;
    const float den_u = a.eps[i] * a.c_out + xin;
    const float den_c = a.eps[n + i] * a.c_out + xin;
    const float den = den_u + a.cfg_scale * (den_c - den_u);
    float xn = xv;
    switch (a.kind) {
      case CRG_KSTEP_DPM2_2: {
        const float d2 = (xin - den) / a.sigma;
        xn = xv + d2 * a.dt;
        if (a.add_noise) xn = xn + (a.noise[i] * a.s_noise) * a.sigma_up;
        break;
      }
      case CRG_KSTEP_SDE_1: {
        float x2 = a.m[0] * xv - a.m[1] * den;
        if (a.add_noise) x2 = x2 + (a.noise[i] * a.s_noise) * a.sigma_up;
        a.x2[i] = x2;
        continue;  // x is not written
      }
      case CRG_KSTEP_SDE_2M:
      case CRG_KSTEP_SDE_3M: {
        if (a.last) {
          xn = den;
        } else {
          xn = a.a * xv + a.c1 * den;
          if (a.kind == CRG_KSTEP_SDE_2M) {
            if (a.have_old) xn = xn + a.c2 * (den - a.old[0][i]);
          } else if (a.order == 2) {
            const float d = (den - a.old[0][i]) / a.r[0];
            xn = xn + a.phi2 * d;
          } else if (a.order == 3) {
            const float den1 = a.old[0][i];
            const float d10 = (den - den1) / a.r[0];
            const float d11 = (den1 - a.old[1][i]) / a.r[1];
            const float dd = d10 - d11;
            const float d1 = d10 + (dd * a.r[0]) / a.rsum;
            const float d2 = dd / a.rsum;
            xn = (xn + a.phi2 * d1) - a.phi3 * d2;
          }
          if (a.add_noise) xn = xn + ((a.noise[i] * a.p[0]) * a.p[1]) * a.s_noise;
        }
        a.den_out[i] = den;
        break;
      }
      default:
        break;
    }
    a.x[i] = xn;
  }
}
}  // namespace

extern "C" int crg_cfg_kstep(crg_ctx* ctx, void* stream, const crg_kstep_args* args) {
  if (!ctx) return -22;
  CRG_REQUIRE(ctx, args != nullptr, "cfg_kstep: null args");
  const crg_kstep_args& a = *args;
  const int k = a.kind;
  CRG_REQUIRE(ctx, k >= CRG_KSTEP_DPM2_2 && k <= CRG_KSTEP_SDE_3M, "cfg_kstep: unknown kind %d", k);
  CRG_REQUIRE(ctx, a.n > 0 && a.x && a.eps, "cfg_kstep: empty input");
  const bool multistep = k == CRG_KSTEP_SDE_2M || k == CRG_KSTEP_SDE_3M;
  CRG_REQUIRE(ctx, k != CRG_KSTEP_DPM2_2 || a.sigma > 0.f, "cfg_kstep: DPM2_2 divides by sigma, which must be positive (got %g)",
              (double)a.sigma);
  CRG_REQUIRE(ctx, multistep || a.x2, "cfg_kstep: kind %d needs x2", k);
  CRG_REQUIRE(ctx, multistep || (a.x2 != a.x), "cfg_kstep: kind %d: x2 must not alias x", k);
  CRG_REQUIRE(ctx, !multistep || a.den_out, "cfg_kstep: kind %d needs den_out", k);
  CRG_REQUIRE(ctx, !multistep || a.den_out != a.x, "cfg_kstep: kind %d: den_out must not alias x", k);
  crg_kstep_args kargs = a;
  kargs.last = multistep && a.last ? 1 : 0;
  kargs.have_old = k == CRG_KSTEP_SDE_2M && !kargs.last && a.have_old ? 1 : 0;
  kargs.order = k == CRG_KSTEP_SDE_3M && !kargs.last ? a.order : 1;
  if (kargs.last) kargs.add_noise = 0;  // x = den: nothing else is read
  kargs.add_noise = kargs.add_noise ? 1 : 0;
  if (k == CRG_KSTEP_SDE_3M && !kargs.last) {
    CRG_REQUIRE(ctx, a.order >= 1 && a.order <= 3, "cfg_kstep: SDE_3M order %d out of 1..3", a.order);
    CRG_REQUIRE(ctx, a.order < 2 || a.r[0] != 0.f, "cfg_kstep: SDE_3M order %d divides by r0, which must not be 0", a.order);
    CRG_REQUIRE(ctx, a.order < 3 || (a.r[1] != 0.f && a.rsum != 0.f), "cfg_kstep: SDE_3M order 3 divides by r1 and r0 + r1, which must not be 0");
  }
  const int n_old = kargs.have_old ? 1 : (k == CRG_KSTEP_SDE_3M ? kargs.order - 1 : 0);
  for (int h = 0; h < n_old; ++h) {
    CRG_REQUIRE(ctx, a.old[h] != nullptr, "cfg_kstep: kind %d reads old[%d], which is null", k, h);
    CRG_REQUIRE(ctx, a.old[h] != a.den_out, "cfg_kstep: den_out must not alias old[%d]", h);
  }
  CRG_REQUIRE(ctx, !kargs.add_noise || a.noise, "cfg_kstep: add_noise needs a noise tensor");
  for (int h = n_old; h < 2; ++h) kargs.old[h] = nullptr;  // nothing past what the branch reads
  if (!kargs.add_noise) kargs.noise = nullptr;
  if (multistep) kargs.x2 = nullptr; else kargs.den_out = nullptr;
  // a written buffer must not start inside eps or be the noise tensor: another thread reads those
  const float* const written[3] = {kargs.x, k == CRG_KSTEP_SDE_1 ? kargs.x2 : nullptr, kargs.den_out};
  for (const float* w : written)
    CRG_REQUIRE(ctx, !w || ((w < a.eps || w >= a.eps + 2 * a.n) && w != kargs.noise), "cfg_kstep: kind %d writes into eps or noise (alias)", k);
  hipStream_t st = (hipStream_t)stream;
  // both eps halves, the input and one store, plus what the kind adds
  const double words = 4.0 + (k == CRG_KSTEP_DPM2_2 ? 1.0 : 0.0) + (multistep ? 1.0 + n_old : 0.0) +
                       (kargs.add_noise ? 1.0 : 0.0);
  crg_prof_scope ps(ctx, st, CRG_K_ELEMENTWISE, (k == CRG_KSTEP_SDE_3M && kargs.order == 3 ? 22.0 : 12.0) * a.n, 4.0 * a.n * words);
  hipLaunchKernelGGL(cfg_kstep_kernel, dim3(grid_for(a.n)), dim3(256), 0, st, kargs);
  CRG_CHECK_LAUNCH(ctx, "cfg_kstep");
  return 0;
}

namespace {
// Bilinear upscale (align_corners = False) of NCHW fp32 planes fused with the forward diffusion of the result (see include/crg_hip.h).
// The source rows / columns and their weights come from host-built tables (ATen's area_pixel_compute_source_index arithmetic in fp32);
// the blend is horizontal, then vertical, and everything after it one fp32 rounding per operation (no FMA contraction).  Table indices
// are clamped to the source plane, so a wrong table gives wrong values, never an out-of-bounds read.
__global__ __launch_bounds__(256) void resize_noise_kernel(const float* __restrict__ x, const float* __restrict__ noise,
                                                           float* __restrict__ out, long n, int h, int w, int H, int W,
                                                           const int* __restrict__ yi, const float* __restrict__ yw,
                                                           const int* __restrict__ xi, const float* __restrict__ xw, float a, float s,
                                                           float d) {
#pragma clang fp contract(off)
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
    const int ox = (int)(i % W);
    const long r = i / W;
    const int oy = (int)(r % H);
    const long plane = r / H;
    const int y0 = min(max(yi[oy], 0), h - 1), y1 = min(max(yi[H + oy], 0), h - 1);
    const int x0 = min(max(xi[ox], 0), w - 1), x1 = min(max(xi[W + ox], 0), w - 1);
    const float wy0 = yw[oy], wy1 = yw[H + oy], wx0 = xw[ox], wx1 = xw[W + ox];
    const float* p = x + plane * ((long)h * w);
    const float top = wx0 * p[(long)y0 * w + x0] + wx1 * p[(long)y0 * w + x1];
    const float bot = wx0 * p[(long)y1 * w + x0] + wx1 * p[(long)y1 * w + x1];
    float v = a * (wy0 * top + wy1 * bot);
    if (noise) v = v + s * noise[i];
    out[i] = v / d;
  }
}
}  // namespace

extern "C" int crg_resize_noise(crg_ctx* ctx, void* stream, const void* x, const void* noise, void* out, int64_t planes, int h, int w,
                                int H, int W, const int* y_idx, const float* y_wt, const int* x_idx, const float* x_wt, float a, float s,
                                float d) {
  if (!ctx) return -22;
  CRG_REQUIRE(ctx, x && out && y_idx && y_wt && x_idx && x_wt, "resize_noise: null pointer");
  CRG_REQUIRE(ctx, x != out && noise != out, "resize_noise: out must not alias x or noise");
  CRG_REQUIRE(ctx, planes > 0 && h > 0 && w > 0 && H > 0 && W > 0, "resize_noise: empty shape (%lld planes, %dx%d -> %dx%d)",
              (long long)planes, h, w, H, W);
  CRG_REQUIRE(ctx, d != 0.f, "resize_noise: the divisor must not be 0");
  const int64_t n = planes * H * W;
  hipStream_t st = (hipStream_t)stream;
  crg_prof_scope ps(ctx, st, CRG_K_ELEMENTWISE, 11.0 * n, 4.0 * (n * (noise ? 2 : 1) + planes * h * w));
  hipLaunchKernelGGL(resize_noise_kernel, dim3(grid_for(n)), dim3(256), 0, st, (const float*)x, (const float*)noise, (float*)out, (long)n, h,
                     w, H, W, y_idx, y_wt, x_idx, x_wt, a, s, d);
  CRG_CHECK_LAUNCH(ctx, "resize_noise");
  return 0;
}

namespace {
// PIL's 8-bit two-pass resize of a window (see include/crg_hip.h).  One block per 64 x 32 output tile of one (image, channel) plane.
// The source rows the tile's vertical taps read are walked in chunks of RS_CH rows: the horizontal pass of a chunk goes to LDS as
// uint8 (PIL clips between the passes), then every thread adds the chunk's share of the vertical taps of its 4 x 2 output pixels to
// integer accumulators in registers - so ksize is a run-time value and LDS is 2 KiB whatever the scale.  A thread's four pixels of a
// row are consecutive columns: one 32-bit LDS read per vertical tap, one 16-byte (fp32) or 4-byte (uint8) store per row.
constexpr int RS_TX = 64, RS_TY = 32, RS_CH = 32, RS_BITS = 22;

template <bool U8>
__device__ __forceinline__ int rs_load(const void* p, long off) {
  if (U8) return ((const unsigned char*)p)[off];
  const float s = fminf(fmaxf(((const float*)p)[off], 0.f), 1.f);
  return (int)(255.0f * s);
}
__device__ __forceinline__ int rs_clip8(int acc) { return min(max(acc >> RS_BITS, 0), 255); }

template <bool SU8, bool DU8>
__global__ __launch_bounds__(256) void resample_u8_kernel(const crg_resample_args a) {
#pragma clang fp contract(off)
  __shared__ unsigned int t_lds[RS_CH * (RS_TX / 4)];
  unsigned char* t8 = reinterpret_cast<unsigned char*>(t_lds);
  const int tid = threadIdx.x;
  const int X0 = blockIdx.x * RS_TX, Y0 = blockIdx.y * RS_TY;
  const int n = blockIdx.z / a.C, c = blockIdx.z % a.C;
  const long sbase = n * a.src_sn + c * a.src_sc + a.y0 * a.src_sy + a.x0 * a.src_sx;
  // the tile's source rows [rlo, rhi): first row's ymin .. last row's ymin + count (bounds do not decrease)
  const int Yl = min(Y0 + RS_TY, a.H) - 1;
  const int rlo = min(max(a.y_bounds[2 * Y0], 0), a.h);
  int rhi = min(max(a.y_bounds[2 * Yl], 0), a.h);
  rhi += min(max(a.y_bounds[2 * Yl + 1], 0), min(a.ksize_y, a.h - rhi));
  // horizontal pass: column hc of rows hr, hr + 4, ...
  const int hc = tid & (RS_TX - 1), hr = tid >> 6;
  const int hX = min(X0 + hc, a.W - 1);
  const int hxmin = min(max(a.x_bounds[2 * hX], 0), a.w);
  const int hxcnt = min(max(a.x_bounds[2 * hX + 1], 0), min(a.ksize_x, a.w - hxmin));
  const int* hk = a.kx + (long)hX * a.ksize_x;
  // vertical pass: columns vx .. vx + 3 of rows Y0 + vy and Y0 + vy + 16
  const int vq = tid & 15, vy = tid >> 4;
  int vmin[2], vend[2], acc[2][4];
  const int* vk[2];
#pragma unroll
  for (int r = 0; r < 2; ++r) {
    const int Y = min(Y0 + vy + 16 * r, a.H - 1);
    vmin[r] = min(max(a.y_bounds[2 * Y], 0), a.h);
    vend[r] = vmin[r] + min(max(a.y_bounds[2 * Y + 1], 0), min(a.ksize_y, a.h - vmin[r]));
    vk[r] = a.ky + (long)Y * a.ksize_y - vmin[r];
#pragma unroll
    for (int e = 0; e < 4; ++e) acc[r][e] = 1 << (RS_BITS - 1);
  }
  for (int cs = rlo; cs < rhi; cs += RS_CH) {
    int h[RS_CH / 4];
    long roff[RS_CH / 4];
#pragma unroll
    for (int i = 0; i < RS_CH / 4; ++i) {
      h[i] = 1 << (RS_BITS - 1);
      roff[i] = sbase + (long)min(cs + hr + 4 * i, rhi - 1) * a.src_sy + (long)hxmin * a.src_sx;  // rows past rhi: computed, never read
    }
    for (int j = 0; j < hxcnt; ++j) {
      const int k = hk[j];
#pragma unroll
      for (int i = 0; i < RS_CH / 4; ++i) h[i] += rs_load<SU8>(a.src, roff[i] + j * a.src_sx) * k;
    }
#pragma unroll
    for (int i = 0; i < RS_CH / 4; ++i) t8[(hr + 4 * i) * RS_TX + hc] = (unsigned char)rs_clip8(h[i]);
    __syncthreads();
#pragma unroll
    for (int r = 0; r < 2; ++r) {
      const int lo = max(vmin[r], cs), hi = min(vend[r], min(cs + RS_CH, rhi));
      for (int j = lo; j < hi; ++j) {
        const int k = vk[r][j];
        const unsigned int u = t_lds[(j - cs) * (RS_TX / 4) + vq];
#pragma unroll
        for (int e = 0; e < 4; ++e) acc[r][e] += (int)((u >> (8 * e)) & 255u) * k;
      }
    }
    __syncthreads();
  }
  const int X = X0 + 4 * vq;
  if (X >= a.W) return;
#pragma unroll
  for (int r = 0; r < 2; ++r) {
    const int Y = Y0 + vy + 16 * r;
    if (Y >= a.H) continue;
    const long doff = n * a.dst_sn + c * a.dst_sc + (long)(a.oy + Y) * a.dst_sy + (long)(a.ox + X) * a.dst_sx;
    int v[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = rs_clip8(acc[r][e]);
    const bool row4 = X + 3 < a.W && a.dst_sx == 1;
    if (DU8) {
      unsigned char* d = (unsigned char*)a.dst + doff;
      if (row4 && ((uintptr_t)d & 3) == 0) {
        *reinterpret_cast<unsigned int*>(d) = (unsigned)v[0] | ((unsigned)v[1] << 8) | ((unsigned)v[2] << 16) | ((unsigned)v[3] << 24);
      } else {
        for (int e = 0; e < 4 && X + e < a.W; ++e) d[e * a.dst_sx] = (unsigned char)v[e];
      }
    } else {
      float* d = (float*)a.dst + doff;
      float f[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float u = (float)v[e] / 255.0f;
        f[e] = a.out_a * u + a.out_b;
      }
      if (row4 && ((uintptr_t)d & 15) == 0) {
        *reinterpret_cast<f32x4*>(d) = f32x4{f[0], f[1], f[2], f[3]};
      } else {
        for (int e = 0; e < 4 && X + e < a.W; ++e) d[e * a.dst_sx] = f[e];
      }
    }
  }
}

// every destination pixel outside the result's rectangle <- the fill value (the two launches write disjoint pixels)
template <bool DU8>
__global__ __launch_bounds__(256) void resample_fill_kernel(const crg_resample_args a, long total) {
  const unsigned char fb = (unsigned char)min(max((int)a.fill_value, 0), 255);
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
    const int x = (int)(i % a.dst_w);
    const long r = i / a.dst_w;
    const int y = (int)(r % a.dst_h);
    const long plane = r / a.dst_h;
    if (x >= a.ox && x < a.ox + a.W && y >= a.oy && y < a.oy + a.H) continue;
    const long doff = (plane / a.C) * a.dst_sn + (plane % a.C) * a.dst_sc + (long)y * a.dst_sy + (long)x * a.dst_sx;
    if (DU8) ((unsigned char*)a.dst)[doff] = fb;
    else ((float*)a.dst)[doff] = a.fill_value;
  }
}
}  // namespace

extern "C" int crg_resample_u8(crg_ctx* ctx, void* stream, const crg_resample_args* args) {
  if (!ctx) return -22;
  CRG_REQUIRE(ctx, args != nullptr, "resample_u8: null args");
  const crg_resample_args& a = *args;
  CRG_REQUIRE(ctx, a.src && a.dst, "resample_u8: null source or destination");
  CRG_REQUIRE(ctx, a.kx && a.x_bounds && a.ky && a.y_bounds, "resample_u8: null coefficient or bounds table");
  CRG_REQUIRE(ctx, (a.src_u8 == 0 || a.src_u8 == 1) && (a.dst_u8 == 0 || a.dst_u8 == 1), "resample_u8: src_u8 / dst_u8 must be 0 or 1 (got %d, %d)",
              a.src_u8, a.dst_u8);
  CRG_REQUIRE(ctx, a.N > 0 && a.C > 0 && (int64_t)a.N * a.C <= 65535, "resample_u8: N * C = %d * %d must be in 1..65535", a.N, a.C);
  CRG_REQUIRE(ctx, a.src_h > 0 && a.src_w > 0 && a.dst_h > 0 && a.dst_w > 0, "resample_u8: empty image (source %dx%d, destination %dx%d)",
              a.src_h, a.src_w, a.dst_h, a.dst_w);
  CRG_REQUIRE(ctx, a.w > 0 && a.h > 0 && a.x0 >= 0 && a.y0 >= 0 && a.x0 <= a.src_w - a.w && a.y0 <= a.src_h - a.h,
              "resample_u8: window (x %d, y %d, w %d, h %d) is empty or outside the %dx%d source", a.x0, a.y0, a.w, a.h, a.src_h, a.src_w);
  CRG_REQUIRE(ctx, a.W > 0 && a.H > 0 && a.ox >= 0 && a.oy >= 0 && a.ox <= a.dst_w - a.W && a.oy <= a.dst_h - a.H,
              "resample_u8: result %dx%d at (x %d, y %d) is empty or outside the %dx%d destination", a.H, a.W, a.ox, a.oy, a.dst_h, a.dst_w);
  CRG_REQUIRE(ctx, a.W <= 65535 * RS_TX && a.H <= 65535 * RS_TY, "resample_u8: result %dx%d is too large", a.H, a.W);
  CRG_REQUIRE(ctx, a.ksize_x > 0 && a.ksize_y > 0, "resample_u8: ksize must be positive (got %d, %d)", a.ksize_x, a.ksize_y);
  CRG_REQUIRE(ctx, a.src_sx > 0 && a.src_sy > 0 && a.src_sn >= 0 && a.src_sc >= 0, "resample_u8: source strides must be positive (n and c: not negative)");
  CRG_REQUIRE(ctx, a.dst_sx > 0 && a.dst_sy > 0 && (a.dst_sn > 0 || a.N == 1) && a.dst_sn >= 0 && (a.dst_sc > 0 || a.C == 1) && a.dst_sc >= 0,
              "resample_u8: destination strides must be positive");
  CRG_REQUIRE(ctx, a.dst_u8 || (a.out_a == a.out_a && a.out_b == a.out_b), "resample_u8: out_a / out_b is NaN");
  CRG_REQUIRE(ctx, !a.fill || a.fill_value == a.fill_value, "resample_u8: the fill value is NaN");
  CRG_REQUIRE(ctx, !a.fill || !a.dst_u8 || (a.fill_value >= 0.f && a.fill_value <= 255.f), "resample_u8: the fill of an uint8 destination must be in 0..255 (got %g)",
              (double)a.fill_value);
  // byte intervals the launch reads (the window) and writes (the rectangle, or with fill the whole destination)
  const int64_t se = a.src_u8 ? 1 : 4, de = a.dst_u8 ? 1 : 4;
  const char* s0 = (const char*)a.src + se * (a.y0 * a.src_sy + a.x0 * a.src_sx);
  const char* s1 = s0 + se * ((a.N - 1) * a.src_sn + (a.C - 1) * a.src_sc + (a.h - 1) * a.src_sy + (a.w - 1) * a.src_sx + 1);
  const int dy = a.fill ? 0 : a.oy, dx = a.fill ? 0 : a.ox, dh = a.fill ? a.dst_h : a.H, dw = a.fill ? a.dst_w : a.W;
  const char* d0 = (const char*)a.dst + de * (dy * a.dst_sy + dx * a.dst_sx);
  const char* d1 = d0 + de * ((a.N - 1) * a.dst_sn + (a.C - 1) * a.dst_sc + (dh - 1) * a.dst_sy + (dw - 1) * a.dst_sx + 1);
  CRG_REQUIRE(ctx, s1 <= d0 || d1 <= s0, "resample_u8: source and destination overlap");
  hipStream_t st = (hipStream_t)stream;
  const double planes = (double)a.N * a.C, px = planes * a.H * a.W;
  crg_prof_scope ps(ctx, st, CRG_K_ELEMENTWISE, 2.0 * px * (a.ksize_x * 0.5 + a.ksize_y),
                    planes * ((double)se * a.h * a.w + (double)de * (a.fill ? (double)a.dst_h * a.dst_w : (double)a.H * a.W)));
  const dim3 grid((a.W + RS_TX - 1) / RS_TX, (a.H + RS_TY - 1) / RS_TY, a.N * a.C);
  if (a.src_u8 && a.dst_u8) hipLaunchKernelGGL((resample_u8_kernel<true, true>), grid, dim3(256), 0, st, a);
  else if (a.src_u8) hipLaunchKernelGGL((resample_u8_kernel<true, false>), grid, dim3(256), 0, st, a);
  else if (a.dst_u8) hipLaunchKernelGGL((resample_u8_kernel<false, true>), grid, dim3(256), 0, st, a);
  else hipLaunchKernelGGL((resample_u8_kernel<false, false>), grid, dim3(256), 0, st, a);
  CRG_CHECK_LAUNCH(ctx, "resample_u8");
  if (a.fill && (a.W < a.dst_w || a.H < a.dst_h)) {
    const long total = (long)a.N * a.C * a.dst_h * a.dst_w;
    if (a.dst_u8) hipLaunchKernelGGL(resample_fill_kernel<true>, dim3(grid_for(total)), dim3(256), 0, st, a, total);
    else hipLaunchKernelGGL(resample_fill_kernel<false>, dim3(grid_for(total)), dim3(256), 0, st, a, total);
    CRG_CHECK_LAUNCH(ctx, "resample_u8 (fill)");
  }
  return 0;
}

extern "C" int crg_axpby(crg_ctx* ctx, void* stream, const void* x, void* y, int64_t n, float a, float b, int dtype) {
  if (!ctx) return -22;
  CRG_REQUIRE(ctx, n > 0, "axpby: empty");
  hipStream_t st = (hipStream_t)stream;
  crg_prof_scope ps(ctx, st, CRG_K_ELEMENTWISE, 3.0 * n, 3.0 * n * crg_dtype_size(dtype));
  if (dtype == CRG_F32)
    hipLaunchKernelGGL(axpby_kernel<float>, dim3(grid_for(n)), dim3(256), 0, st, (const float*)x, (float*)y, (long)n, a, b);
  else if (dtype == CRG_BF16)
    hipLaunchKernelGGL(axpby_kernel<bf16>, dim3(grid_for(n)), dim3(256), 0, st, (const bf16*)x, (bf16*)y, (long)n, a, b);
  else
    return crg_fail(ctx, -22, "axpby: dtype %d unsupported", dtype);
  CRG_CHECK_LAUNCH(ctx, "axpby");
  return 0;
}
