// Data movements of the FILM frame interpolator (frame_interpolation_pytorch: util.py, feature_extractor.py, pyramid_flow_estimator.py)
// on channels-last fp32 rows: pixel (n, y, x) of a tensor is row (n H + y) W + x, `ld` elements apart, its channels consecutive.
//
// Every kernel that writes takes a destination row stride ld >= C and a pointer that already carries the channel offset: the reference's
// torch.cat's are writes into column slices of one buffer, and a kernel touches the C channels of its slice only.  All of them are HBM
// streams or gathers: 16-byte accesses where pointer, stride and C allow (V = 4), one element per lane otherwise; plain vector stores.
//
// crg_film_warp:    backward warp by a flow (util.warp once its normalise / grid_sample round trip is undone): bilinear lookup at
//                   (x + s fx, y + s fy), coordinates clamped to the image (padding_mode 'border', align_corners False), s per sample.
//                   LPP <= 64 lanes share a pixel; EACH lane reads the pixel's flow (one broadcast access) and computes the four
//                   weights once, then walks its share of the channels: the weights are per lane, not per channel and not per pixel.
// crg_film_pool2:   F.avg_pool2d(x, 2, 2); odd sizes floor.
// crg_film_flow_up: residual + F.interpolate(2 v, exactly twice the size, 'bilinear') on two channels.
// crg_film_act:     LeakyReLU (times a per-sample scalar) of a conv output as fp32 and / or (hi, lo) half-type planes, optionally with
//                   the 2 x 2 mean of the activation in the same pass.
#include "crg_common.h"

namespace {

__device__ __forceinline__ void film_split(float v, bf16& hi, bf16& lo) {
  hi = (bf16)v;
  lo = (bf16)(v - (float)hi);
}

// ---- warp ---------------------------------------------------------------------------------------------------------------------------
struct FilmWarpP {
  const float* src; long ld_s;
  const float* flow; long ld_f;
  const float* scale;
  float* dst; long ld_d;
  bf16* hi; bf16* lo; long ld_p;
  long pixels;
  int H, W, C, lpp_log2;
};

// V: channels per access of the source (4: src, ld_s 16-byte aligned and C % 4 == 0).  VD: the destinations take the same accesses.
template <int V, bool VD>
__global__ __launch_bounds__(256) void film_warp_kernel(const FilmWarpP p) {
  const long gid = (long)blockIdx.x * 256 + threadIdx.x;
  const long pix = gid >> p.lpp_log2;
  const int sub = (int)(gid & ((1 << p.lpp_log2) - 1));
  if (pix >= p.pixels) return;
  const int x = (int)(pix % p.W);
  const long r = pix / p.W;
  const int y = (int)(r % p.H);
  const long n = r / p.H;
  const float s = p.scale ? p.scale[n] : 1.0f;
  const float* f = p.flow + pix * p.ld_f;
  // clamped source position; a NaN flow lands on the border (fmin / fmax return the other operand), never outside the image
  const float sx = __builtin_fmaxf(__builtin_fminf(__builtin_fmaf(s, f[0], (float)x), (float)(p.W - 1)), 0.0f);
  const float sy = __builtin_fmaxf(__builtin_fminf(__builtin_fmaf(s, f[1], (float)y), (float)(p.H - 1)), 0.0f);
  const float fx0 = __builtin_floorf(sx), fy0 = __builtin_floorf(sy);
  const float ax = sx - fx0, ay = sy - fy0;
  const int x0 = (int)fx0, y0 = (int)fy0;
  const int x1 = x0 + 1 < p.W ? x0 + 1 : p.W - 1, y1 = y0 + 1 < p.H ? y0 + 1 : p.H - 1;
  const float w00 = (1.0f - ax) * (1.0f - ay), w01 = ax * (1.0f - ay), w10 = (1.0f - ax) * ay, w11 = ax * ay;
  const bool whole = ax == 0.0f && ay == 0.0f;  // an integral position is the source pixel itself, bit for bit
  const long img = n * p.H;
  const float* s00 = p.src + ((img + y0) * p.W + x0) * p.ld_s;
  const float* s01 = p.src + ((img + y0) * p.W + x1) * p.ld_s;
  const float* s10 = p.src + ((img + y1) * p.W + x0) * p.ld_s;
  const float* s11 = p.src + ((img + y1) * p.W + x1) * p.ld_s;
  const int step = V << p.lpp_log2;
  for (int c = sub * V; c < p.C; c += step) {
    float v[V];
    if constexpr (V == 4) {
      const f32x4 a = *reinterpret_cast<const f32x4*>(s00 + c), b = *reinterpret_cast<const f32x4*>(s01 + c);
      const f32x4 d = *reinterpret_cast<const f32x4*>(s10 + c), e = *reinterpret_cast<const f32x4*>(s11 + c);
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const float t = __builtin_fmaf(w11, e[i], __builtin_fmaf(w10, d[i], __builtin_fmaf(w01, b[i], w00 * a[i])));
        v[i] = whole ? a[i] : t;
      }
    } else {
      const float a = s00[c];
      const float t = __builtin_fmaf(w11, s11[c], __builtin_fmaf(w10, s10[c], __builtin_fmaf(w01, s01[c], w00 * a)));
      v[0] = whole ? a : t;
    }
    if (p.dst) {
      float* o = p.dst + pix * p.ld_d + c;
      if constexpr (V == 4 && VD) {
        *reinterpret_cast<f32x4*>(o) = f32x4{v[0], v[1], v[2], v[3]};
      } else {
#pragma unroll
        for (int i = 0; i < V; ++i) o[i] = v[i];
      }
    }
    if (p.hi) {
      bf16 h[V], l[V];
#pragma unroll
      for (int i = 0; i < V; ++i) film_split(v[i], h[i], l[i]);
      bf16* oh = p.hi + pix * p.ld_p + c;
      bf16* ol = p.lo + pix * p.ld_p + c;
      if constexpr (V == 4 && VD) {
        *reinterpret_cast<bf16x4*>(oh) = bf16x4{h[0], h[1], h[2], h[3]};
        *reinterpret_cast<bf16x4*>(ol) = bf16x4{l[0], l[1], l[2], l[3]};
      } else {
#pragma unroll
        for (int i = 0; i < V; ++i) {
          oh[i] = h[i];
          ol[i] = l[i];
        }
      }
    }
  }
}

// ---- 2 x 2 average pooling ------------------------------------------------------------------------------------------------------------
struct FilmPoolP {
  const float* src; long ld_s;
  float* dst; long ld_d;
  long items;  // N Ho Wo (C / V)
  int H, W, Ho, Wo, CV;
};

template <int V>
__global__ __launch_bounds__(256) void film_pool2_kernel(const FilmPoolP p) {
  const long gid = (long)blockIdx.x * 256 + threadIdx.x;
  if (gid >= p.items) return;
  const int c = (int)(gid % p.CV) * V;
  const long op = gid / p.CV;
  const int xo = (int)(op % p.Wo);
  const long r = op / p.Wo;
  const int yo = (int)(r % p.Ho);
  const long n = r / p.Ho;
  const float* a = p.src + ((n * p.H + 2 * yo) * p.W + 2 * xo) * p.ld_s + c;
  const float* b = a + (long)p.W * p.ld_s;
  float* o = p.dst + op * p.ld_d + c;
  if constexpr (V == 4) {
    const f32x4 v = (((*reinterpret_cast<const f32x4*>(a) + *reinterpret_cast<const f32x4*>(a + p.ld_s)) + *reinterpret_cast<const f32x4*>(b)) +
                     *reinterpret_cast<const f32x4*>(b + p.ld_s)) * 0.25f;
    *reinterpret_cast<f32x4*>(o) = v;
  } else {
    o[0] = (((a[0] + a[p.ld_s]) + b[0]) + b[p.ld_s]) * 0.25f;
  }
}

// ---- x 2 bilinear flow upsampling + residual --------------------------------------------------------------------------------------------
struct FilmUpP {
  const float* v; long ld_v;
  const float* res; long ld_r;
  float* dst; long ld_d;
  long pixels;  // N 2h 2w
  int h, w;
};

// Output index o of an exact x 2 (align_corners False) reads source position o / 2 - 1 / 4, clamped at 0: rows i0 and i1 = min(i0 + 1,
// n - 1) with weights (1 - l, l), l = 3 / 4 for even o > 0, 1 / 4 for odd o, 0 for o = 0.
__device__ __forceinline__ void film_up_taps(int o, int n, int& i0, int& i1, float& l) {
  const bool odd = o & 1;
  i0 = odd ? o >> 1 : (o > 0 ? (o >> 1) - 1 : 0);
  i1 = i0 + (i0 < n - 1 ? 1 : 0);
  l = odd ? 0.25f : (o > 0 ? 0.75f : 0.0f);
}

__global__ __launch_bounds__(256) void film_flow_up_kernel(const FilmUpP p) {
  const long pix = (long)blockIdx.x * 256 + threadIdx.x;
  if (pix >= p.pixels) return;
  const int W2 = 2 * p.w, H2 = 2 * p.h;
  const int x = (int)(pix % W2);
  const long r = pix / W2;
  const int y = (int)(r % H2);
  const long n = r / H2;
  int x0, x1, y0, y1;
  float lx, ly;
  film_up_taps(x, p.w, x0, x1, lx);
  film_up_taps(y, p.h, y0, y1, ly);
  const float* r0 = p.v + (n * p.h + y0) * p.w * p.ld_v;
  const float* r1 = p.v + (n * p.h + y1) * p.w * p.ld_v;
  float* o = p.dst + pix * p.ld_d;
#pragma unroll
  for (int c = 0; c < 2; ++c) {
    const float a = 2.0f * r0[x0 * p.ld_v + c], b = 2.0f * r0[x1 * p.ld_v + c];
    const float d = 2.0f * r1[x0 * p.ld_v + c], e = 2.0f * r1[x1 * p.ld_v + c];
    const float up = (1.0f - ly) * ((1.0f - lx) * a + lx * b) + ly * ((1.0f - lx) * d + lx * e);
    o[c] = p.res ? p.res[pix * p.ld_r + c] + up : up;
  }
}

// ---- LeakyReLU (+ planes, + pooled) -----------------------------------------------------------------------------------------------------
struct FilmActP {
  const float* x; long ld_x;
  float* y; long ld_y;
  bf16* hi; bf16* lo; long ld_p;
  float* pool; long ld_q;
  const float* scale;
  long items;  // N Hq Wq (C / V): Hq x Wq quads of 2 x 2 pixels when pooling, pixels otherwise
  int H, W, Hq, Wq, CV;
  float slope;
};

template <int V, bool POOL>
__global__ __launch_bounds__(256) void film_act_kernel(const FilmActP p) {
  const long gid = (long)blockIdx.x * 256 + threadIdx.x;
  if (gid >= p.items) return;
  const int c = (int)(gid % p.CV) * V;
  const long q = gid / p.CV;
  constexpr int Q = POOL ? 2 : 1;
  const int xq = (int)(q % p.Wq);
  const long r = q / p.Wq;
  const int yq = (int)(r % p.Hq);
  const long n = r / p.Hq;
  const float s = p.scale ? p.scale[n] : 1.0f;
  float sum[V];
#pragma unroll
  for (int i = 0; i < V; ++i) sum[i] = 0.0f;
#pragma unroll
  for (int dy = 0; dy < Q; ++dy)
#pragma unroll
    for (int dx = 0; dx < Q; ++dx) {
      const int yy = Q * yq + dy, xx = Q * xq + dx;
      if (yy >= p.H || xx >= p.W) continue;  // the last row / column of an odd size: written, not pooled
      const long pix = (n * p.H + yy) * p.W + xx;
      float v[V];
      if constexpr (V == 4) {
        const f32x4 t = *reinterpret_cast<const f32x4*>(p.x + pix * p.ld_x + c);
#pragma unroll
        for (int i = 0; i < 4; ++i) v[i] = t[i];
      } else {
        v[0] = p.x[pix * p.ld_x + c];
      }
#pragma unroll
      for (int i = 0; i < V; ++i) {
        v[i] = v[i] >= 0.0f ? v[i] : v[i] * p.slope;
        if (p.scale) v[i] *= s;
        sum[i] += v[i];
      }
      if (p.y) {
        float* o = p.y + pix * p.ld_y + c;
        if constexpr (V == 4) {
          *reinterpret_cast<f32x4*>(o) = f32x4{v[0], v[1], v[2], v[3]};
        } else {
          o[0] = v[0];
        }
      }
      if (p.hi) {
        bf16 h[V], l[V];
#pragma unroll
        for (int i = 0; i < V; ++i) film_split(v[i], h[i], l[i]);
        bf16* oh = p.hi + pix * p.ld_p + c;
        bf16* ol = p.lo + pix * p.ld_p + c;
        if constexpr (V == 4) {
          *reinterpret_cast<bf16x4*>(oh) = bf16x4{h[0], h[1], h[2], h[3]};
          *reinterpret_cast<bf16x4*>(ol) = bf16x4{l[0], l[1], l[2], l[3]};
        } else {
          oh[0] = h[0];
          ol[0] = l[0];
        }
      }
    }
  if constexpr (POOL) {
    if (yq < p.H / 2 && xq < p.W / 2) {
      float* o = p.pool + ((n * (p.H / 2) + yq) * (p.W / 2) + xq) * p.ld_q + c;
      if constexpr (V == 4) {
        *reinterpret_cast<f32x4*>(o) = f32x4{sum[0], sum[1], sum[2], sum[3]} * 0.25f;
      } else {
        o[0] = sum[0] * 0.25f;
      }
    }
  }
}

inline bool al16(const void* p) { return ((uintptr_t)p & 15) == 0; }
inline bool al8(const void* p) { return ((uintptr_t)p & 7) == 0; }
inline bool grid_ok(long items) { return items > 0 && (items + 255) / 256 < (1L << 31); }
}  // namespace

extern "C" int crg_film_warp(crg_ctx* ctx, void* stream, const crg_film_warp_args* a) {
  if (!ctx) return -22;
  CRG_REQUIRE(ctx, a && a->src && a->flow && (a->dst || a->hi), "film_warp: bad arguments");
  CRG_REQUIRE(ctx, (a->hi == nullptr) == (a->lo == nullptr), "film_warp: the planes come as a pair");
  CRG_REQUIRE(ctx, a->N >= 1 && a->H >= 1 && a->W >= 1 && a->C >= 1, "film_warp: empty problem N=%d H=%d W=%d C=%d", a->N, a->H, a->W, a->C);
  CRG_REQUIRE(ctx, a->ld_src >= a->C && a->ld_flow >= 2 && (!a->dst || a->ld_dst >= a->C) && (!a->hi || a->ld_planes >= a->C),
              "film_warp: a row stride is smaller than its channel count (C=%d)", a->C);
  CRG_REQUIRE(ctx, (((uintptr_t)a->src | (uintptr_t)a->flow | (uintptr_t)a->dst | (uintptr_t)a->scale) & 3) == 0 && (((uintptr_t)a->hi | (uintptr_t)a->lo) & 1) == 0,
              "film_warp: misaligned pointer");
  const long pixels = (long)a->N * a->H * a->W;
  const bool vs = a->C % 4 == 0 && al16(a->src) && a->ld_src % 4 == 0;
  const bool vd = vs && (!a->dst || (al16(a->dst) && a->ld_dst % 4 == 0)) && (!a->hi || (al8(a->hi) && al8(a->lo) && a->ld_planes % 4 == 0));
  const int chunks = vs ? a->C / 4 : a->C;
  int lg = 0;
  while ((1 << lg) < chunks && lg < 6) ++lg;
  CRG_REQUIRE(ctx, grid_ok(pixels << lg), "film_warp: %ld pixels exceed the grid", pixels);
  FilmWarpP p = {a->src, a->ld_src, a->flow, a->ld_flow, a->scale, a->dst, a->ld_dst, (bf16*)a->hi, (bf16*)a->lo, a->ld_planes, pixels, a->H, a->W, a->C, lg};
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)(((pixels << lg) + 255) / 256));
  crg_prof_scope ps(ctx, st, CRG_K_ELEMENTWISE, 8.0 * pixels * a->C, (double)pixels * (4.0 * a->C * 4 + 8 + (a->dst ? 4.0 : 0.0) * a->C + (a->hi ? 4.0 : 0.0) * a->C));
  if (vd)
    hipLaunchKernelGGL((film_warp_kernel<4, true>), grid, dim3(256), 0, st, p);
  else if (vs)
    hipLaunchKernelGGL((film_warp_kernel<4, false>), grid, dim3(256), 0, st, p);
  else
    hipLaunchKernelGGL((film_warp_kernel<1, false>), grid, dim3(256), 0, st, p);
  CRG_CHECK_LAUNCH(ctx, "film_warp");
  return 0;
}

extern "C" int crg_film_pool2(crg_ctx* ctx, void* stream, const float* src, int64_t ld_src, float* dst, int64_t ld_dst, int N, int H, int W, int C) {
  if (!ctx) return -22;
  CRG_REQUIRE(ctx, src && dst, "film_pool2: bad arguments");
  CRG_REQUIRE(ctx, N >= 1 && H >= 2 && W >= 2 && C >= 1, "film_pool2: empty problem N=%d H=%d W=%d C=%d", N, H, W, C);
  CRG_REQUIRE(ctx, ld_src >= C && ld_dst >= C, "film_pool2: a row stride is smaller than C=%d", C);
  CRG_REQUIRE(ctx, (((uintptr_t)src | (uintptr_t)dst) & 3) == 0, "film_pool2: misaligned pointer");
  const bool v4 = C % 4 == 0 && al16(src) && al16(dst) && ld_src % 4 == 0 && ld_dst % 4 == 0;
  const int V = v4 ? 4 : 1;
  FilmPoolP p = {src, ld_src, dst, ld_dst, (long)N * (H / 2) * (W / 2) * (C / V), H, W, H / 2, W / 2, C / V};
  CRG_REQUIRE(ctx, grid_ok(p.items), "film_pool2: %ld items exceed the grid", p.items);
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)((p.items + 255) / 256));
  crg_prof_scope ps(ctx, st, CRG_K_ELEMENTWISE, 4.0 * p.items * V, 20.0 * p.items * V);
  if (v4)
    hipLaunchKernelGGL((film_pool2_kernel<4>), grid, dim3(256), 0, st, p);
  else
    hipLaunchKernelGGL((film_pool2_kernel<1>), grid, dim3(256), 0, st, p);
  CRG_CHECK_LAUNCH(ctx, "film_pool2");
  return 0;
}

extern "C" int crg_film_flow_up(crg_ctx* ctx, void* stream, const float* v, int64_t ld_v, const float* residual, int64_t ld_res, float* dst, int64_t ld_dst,
                                int N, int h, int w) {
  if (!ctx) return -22;
  CRG_REQUIRE(ctx, v && dst, "film_flow_up: bad arguments");
  CRG_REQUIRE(ctx, N >= 1 && h >= 1 && w >= 1 && h < (1 << 29) && w < (1 << 29), "film_flow_up: bad problem N=%d h=%d w=%d", N, h, w);
  CRG_REQUIRE(ctx, ld_v >= 2 && ld_dst >= 2 && (!residual || ld_res >= 2), "film_flow_up: a row stride is smaller than the two flow channels");
  CRG_REQUIRE(ctx, (((uintptr_t)v | (uintptr_t)residual | (uintptr_t)dst) & 3) == 0, "film_flow_up: misaligned pointer");
  FilmUpP p = {v, ld_v, residual, ld_res, dst, ld_dst, (long)N * 4 * h * w, h, w};
  CRG_REQUIRE(ctx, grid_ok(p.pixels), "film_flow_up: %ld pixels exceed the grid", p.pixels);
  hipStream_t st = (hipStream_t)stream;
  crg_prof_scope ps(ctx, st, CRG_K_ELEMENTWISE, 14.0 * p.pixels, (residual ? 18.0 : 10.0) * p.pixels);
  hipLaunchKernelGGL(film_flow_up_kernel, dim3((unsigned)((p.pixels + 255) / 256)), dim3(256), 0, st, p);
  CRG_CHECK_LAUNCH(ctx, "film_flow_up");
  return 0;
}

extern "C" int crg_film_act(crg_ctx* ctx, void* stream, const crg_film_act_args* a) {
  if (!ctx) return -22;
  CRG_REQUIRE(ctx, a && a->x && (a->y || a->hi || a->pool), "film_act: bad arguments");
  CRG_REQUIRE(ctx, (a->hi == nullptr) == (a->lo == nullptr), "film_act: the planes come as a pair");
  CRG_REQUIRE(ctx, a->N >= 1 && a->H >= 1 && a->W >= 1 && a->C >= 1, "film_act: empty problem N=%d H=%d W=%d C=%d", a->N, a->H, a->W, a->C);
  CRG_REQUIRE(ctx, !a->pool || (a->H >= 2 && a->W >= 2), "film_act: a %d x %d image has no 2 x 2 mean", a->H, a->W);
  CRG_REQUIRE(ctx, a->ld_x >= a->C && (!a->y || a->ld_y >= a->C) && (!a->hi || a->ld_planes >= a->C) && (!a->pool || a->ld_pool >= a->C),
              "film_act: a row stride is smaller than C=%d", a->C);
  CRG_REQUIRE(ctx, (((uintptr_t)a->x | (uintptr_t)a->y | (uintptr_t)a->pool | (uintptr_t)a->scale) & 3) == 0 && (((uintptr_t)a->hi | (uintptr_t)a->lo) & 1) == 0, "film_act: misaligned pointer");
  const bool v4 = a->C % 4 == 0 && al16(a->x) && a->ld_x % 4 == 0 && (!a->y || (al16(a->y) && a->ld_y % 4 == 0)) &&
                  (!a->hi || (al8(a->hi) && al8(a->lo) && a->ld_planes % 4 == 0)) && (!a->pool || (al16(a->pool) && a->ld_pool % 4 == 0));
  const int V = v4 ? 4 : 1;
  const int Hq = a->pool ? (a->H + 1) / 2 : a->H, Wq = a->pool ? (a->W + 1) / 2 : a->W;
  FilmActP p = {a->x, a->ld_x, a->y, a->ld_y, (bf16*)a->hi, (bf16*)a->lo, a->ld_planes, a->pool, a->ld_pool, a->scale, (long)a->N * Hq * Wq * (a->C / V),
                a->H, a->W, Hq, Wq, a->C / V, a->slope};
  CRG_REQUIRE(ctx, grid_ok(p.items), "film_act: %ld items exceed the grid", p.items);
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)((p.items + 255) / 256));
  const double elems = (double)a->N * a->H * a->W * a->C;
  crg_prof_scope ps(ctx, st, CRG_K_ELEMENTWISE, 2.0 * elems, elems * (4.0 + (a->y ? 4.0 : 0.0) + (a->hi ? 4.0 : 0.0) + (a->pool ? 1.0 : 0.0)));
  if (a->pool) {
    if (v4)
      hipLaunchKernelGGL((film_act_kernel<4, true>), grid, dim3(256), 0, st, p);
    else
      hipLaunchKernelGGL((film_act_kernel<1, true>), grid, dim3(256), 0, st, p);
  } else {
    if (v4)
      hipLaunchKernelGGL((film_act_kernel<4, false>), grid, dim3(256), 0, st, p);
    else
      hipLaunchKernelGGL((film_act_kernel<1, false>), grid, dim3(256), 0, st, p);
  }
  CRG_CHECK_LAUNCH(ctx, "film_act");
  return 0;
}
