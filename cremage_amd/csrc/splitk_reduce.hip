// Split-K second passes (gfx950): the kernels that sum the fp32 K-slice slabs of a split-K GEMM / conv launch and finish the output -
// plain, with GroupNorm statistics, with LayerNorm row statistics, or fused with the GroupNorm(+SiLU) behind the conv - and their launch.
#include "gemm_shared.h"

namespace {
using namespace crg_mm;

// Split-K second pass: y = epi(sum_s slab[s] + bias) + cvec + residual, 4 consecutive n per thread.
template <typename YT>
__global__ __launch_bounds__(256) void splitk_reduce_kernel(GemmP p) {
  const int n4 = p.N >> 2;
  const long srows = p.M - p.slab_row0;
  const long total = srows * n4;
  const int bz = blockIdx.y;
  const float* S = p.slab + (long)bz * p.splits * srows * p.N - (long)p.slab_row0 * p.N;
  YT* Y = reinterpret_cast<YT*>(p.y) + (long)bz * p.y_bs;
  const YT* R = p.res ? reinterpret_cast<const YT*>(p.res) + (long)bz * p.r_bs : nullptr;
  for (long idx = (long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long)gridDim.x * 256) {
    const int mr = (int)(idx / n4);
    const int m = mr + p.slab_row0;
    const int n = (int)(idx - (long)mr * n4) * 4;
    f32x4 v = *reinterpret_cast<const f32x4*>(S + (long)m * p.N + n);
    for (int s = 1; s < p.splits; ++s) v += *reinterpret_cast<const f32x4*>(S + ((long)s * srows + m) * p.N + n);
    if (p.bias_mode == CRG_BIAS_COL) v += *reinterpret_cast<const f32x4*>(p.bias + n);
    else if (p.bias_mode == CRG_BIAS_ROW) v += p.bias[m];
    if (p.epi == CRG_EPI_SILU) {
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] = crg_silu_f(v[e]);
    }
    if (p.cvec) v += *reinterpret_cast<const f32x4*>(p.cvec + (long)(m / p.cvec_rows) * p.cvec_ld + n);
    if (R) {
      const YT* rp = R + (long)m * p.ldr + n;
#pragma unroll
      for (int e = 0; e < 4; ++e) v[e] += (float)rp[e];
    }
    YT* yp = Y + (p.up == 2 ? up2_out_row(p, m) : (long)m) * p.ldy + n;
    if ((p.ldy & 3) == 0) {
      if constexpr (sizeof(YT) == 2) {
        bf16x4 o4;
#pragma unroll
        for (int e = 0; e < 4; ++e) o4[e] = (bf16)v[e];
        *reinterpret_cast<bf16x4*>(yp) = o4;
      } else {
        *reinterpret_cast<f32x4*>(yp) = v;
      }
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e) yp[e] = (YT)v[e];
    }
  }
}

// Split-K second pass that ALSO emits the GroupNorm statistics side channel (GemmP::gstat): same arithmetic per element as
// splitk_reduce_kernel, but a block owns a 32-row x 128-column patch - thread = (row lane 0..7: rows 4 rl .. 4 rl + 3, column group
// of 4 channels) - so that the per-channel sums of the rounded outputs over the 32 rows are a fixed-order fold of 8 row lanes
// through LDS.  grid (row blocks, column patches).
template <typename YT>
__global__ __launch_bounds__(256) void splitk_reduce_stats_kernel(GemmP p) {
  __shared__ __attribute__((aligned(16))) float red[8 * 32 * 8];
  const int t = threadIdx.x, cg = t & 31, rl = t >> 5;
  const long srows = p.M - p.slab_row0;
  const float* S = p.slab - (long)p.slab_row0 * p.N;
  YT* Y = reinterpret_cast<YT*>(p.y);
  const YT* R = p.res ? reinterpret_cast<const YT*>(p.res) : nullptr;
  const int n = blockIdx.y * 128 + cg * 4;
  const int mb = p.slab_row0 + blockIdx.x * 32;
  float s1[4] = {0.f, 0.f, 0.f, 0.f}, s2[4] = {0.f, 0.f, 0.f, 0.f};
  if (n < p.N) {
    f32x4 v[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int m = mb + rl * 4 + i;
      const int mc = m < p.M ? m : p.M - 1;  // clamped: the loads stay unconditional, the result of a row past M is dropped
      v[i] = *reinterpret_cast<const f32x4*>(S + (long)mc * p.N + n);
      for (int s = 1; s < p.splits; ++s) v[i] += *reinterpret_cast<const f32x4*>(S + ((long)s * srows + mc) * p.N + n);
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int m = mb + rl * 4 + i;
      if (m >= p.M) continue;
      f32x4 w = v[i];
      if (p.bias_mode == CRG_BIAS_COL) w += *reinterpret_cast<const f32x4*>(p.bias + n);
      else if (p.bias_mode == CRG_BIAS_ROW) w += p.bias[m];
      if (p.epi == CRG_EPI_SILU) {
#pragma unroll
        for (int e = 0; e < 4; ++e) w[e] = crg_silu_f(w[e]);
      }
      if (p.cvec) w += *reinterpret_cast<const f32x4*>(p.cvec + (long)(m / p.cvec_rows) * p.cvec_ld + n);
      if (R) {
        const YT* rp = R + (long)m * p.ldr + n;
#pragma unroll
        for (int e = 0; e < 4; ++e) w[e] += (float)rp[e];
      }
      YT o[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        o[e] = (YT)w[e];
        const float f = (float)o[e];
        s1[e] += f;
        s2[e] += f * f;
      }
      YT* yp = Y + (p.up == 2 ? up2_out_row(p, m) : (long)m) * p.ldy + n;
      if constexpr (sizeof(YT) == 2) *reinterpret_cast<uint2*>(yp) = *reinterpret_cast<const uint2*>(o);
      else *reinterpret_cast<f32x4*>(yp) = *reinterpret_cast<const f32x4*>(o);
    }
  }
  float* q = red + (rl * 32 + cg) * 8;
  *reinterpret_cast<f32x4*>(q) = f32x4{s1[0], s1[1], s1[2], s1[3]};
  *reinterpret_cast<f32x4*>(q + 4) = f32x4{s2[0], s2[1], s2[2], s2[3]};
  __syncthreads();
  if (rl == 0 && n < p.N) {
    f32x4 a = *reinterpret_cast<const f32x4*>(q), b = *reinterpret_cast<const f32x4*>(q + 4);
#pragma unroll
    for (int r2 = 1; r2 < 8; ++r2) {
      a += *reinterpret_cast<const f32x4*>(q + r2 * 32 * 8);
      b += *reinterpret_cast<const f32x4*>(q + r2 * 32 * 8 + 4);
    }
    const long rb = mb >> 5;
    *reinterpret_cast<f32x4*>(p.gstat + rb * p.N + n) = a;
    *reinterpret_cast<f32x4*>(p.gstat + p.gstat_plane + rb * p.N + n) = b;
  }
}

// Split-K second pass that ALSO emits the LayerNorm row statistics (GemmP::rstat) of the finished rows: a wave owns a row at a time (lanes
// stride over its 4-column groups), sums the rounded outputs and their squares, folds the 64 lanes with shuffles (fixed order) and writes
// the whole-row sums into partial 0; the other partials of the row are zeroed (the consumer folds all rstat_parts of them).
__global__ __launch_bounds__(256) void splitk_reduce_rows_kernel(GemmP p) {
  const int n4 = p.N >> 2;
  const long srows = p.M - p.slab_row0;
  const float* S = p.slab - (long)p.slab_row0 * p.N;
  bf16* Y = reinterpret_cast<bf16*>(p.y);
  const bf16* R = reinterpret_cast<const bf16*>(p.res);
  const int lane = threadIdx.x & 63;
  for (int m = p.slab_row0 + blockIdx.x * 4 + (threadIdx.x >> 6); m < p.M; m += gridDim.x * 4) {
    float q1 = 0.f, q2 = 0.f;
    for (int c = lane; c < n4; c += 64) {
      const int n = c * 4;
      f32x4 v = *reinterpret_cast<const f32x4*>(S + (long)m * p.N + n);
      for (int s = 1; s < p.splits; ++s) v += *reinterpret_cast<const f32x4*>(S + ((long)s * srows + m) * p.N + n);
      if (p.bias_mode == CRG_BIAS_COL) v += *reinterpret_cast<const f32x4*>(p.bias + n);
      else if (p.bias_mode == CRG_BIAS_ROW) v += p.bias[m];
      if (R) {
        const bf16x4 r4 = *reinterpret_cast<const bf16x4*>(R + (long)m * p.ldr + n);
#pragma unroll
        for (int e = 0; e < 4; ++e) v[e] += (float)r4[e];
      }
      bf16x4 o4;
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        o4[e] = (bf16)v[e];
        const float f = (float)o4[e];
        q1 += f;
        q2 = __builtin_fmaf(f, f, q2);
      }
      *reinterpret_cast<bf16x4*>(Y + (long)m * p.ldy + n) = o4;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      q1 += __shfl_xor(q1, o);
      q2 += __shfl_xor(q2, o);
    }
    if (lane < p.rstat_parts) *reinterpret_cast<f32x2*>(p.rstat + ((long)m * p.rstat_parts + lane) * 2) = lane == 0 ? f32x2{q1, q2} : f32x2{0.f, 0.f};
  }
}

// Split-K second pass FUSED with the GroupNorm(+SiLU) that consumes the conv's output (openaimodel.py:208 -> :229-231 inside a ResBlock),
// for the small images of the two lowest UNet levels: one block per (sample, group) sums the K slices of its HW x gs slab in slice order,
// adds bias / per-sample vector / residual in the order of splitk_reduce_kernel, rounds to bf16 and stores the raw output, and then
// normalises those very values with the arithmetic of gn_small_kernel (shifted sums, wave shuffles, fixed-order cross-wave fp64
// combine) - bitwise what the reduce kernel followed by the single-launch GroupNorm produce, in one launch and without re-reading y.
template <int VPT>
__global__ __launch_bounds__(256) void splitk_reduce_gn_kernel(GemmP p) {
  __shared__ float red[2][4];
  __shared__ float shift_s;
  const int n = blockIdx.y, g = blockIdx.x, t = threadIdx.x;
  const int C = p.N, HW = p.gn_hw;
  const int gs = C / p.gn_groups, wv = gs >> 3;
  const int c_beg = g * gs;
  const int total = HW * wv;
  const long slice = (long)p.M * p.N;
  const float* S = p.slab;
  bf16* Y = reinterpret_cast<bf16*>(p.y);
  const bf16* R = reinterpret_cast<const bf16*>(p.res);
  crg_vec8<bf16> v[VPT];
  int row[VPT], cv[VPT];
#pragma unroll
  for (int k = 0; k < VPT; ++k) {
    const int i = t + 256 * k;
    row[k] = i / wv;
    cv[k] = i - row[k] * wv;
    if (i < total) {
      const long m = (long)n * HW + row[k];
      const int c = c_beg + cv[k] * 8;
      const float* sp = S + m * p.N + c;
      f32x4 a = *reinterpret_cast<const f32x4*>(sp), b = *reinterpret_cast<const f32x4*>(sp + 4);
      for (int s2 = 1; s2 < p.splits; ++s2) {
        a += *reinterpret_cast<const f32x4*>(sp + s2 * slice);
        b += *reinterpret_cast<const f32x4*>(sp + s2 * slice + 4);
      }
      if (p.bias_mode == CRG_BIAS_COL) {
        a += *reinterpret_cast<const f32x4*>(p.bias + c);
        b += *reinterpret_cast<const f32x4*>(p.bias + c + 4);
      }
      if (p.cvec) {
        const float* cp = p.cvec + (m / p.cvec_rows) * p.cvec_ld + c;
        a += *reinterpret_cast<const f32x4*>(cp);
        b += *reinterpret_cast<const f32x4*>(cp + 4);
      }
      if (R) {
        const bf16x8 r8 = *reinterpret_cast<const bf16x8*>(R + m * p.ldr + c);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          a[e] += (float)r8[e];
          b[e] += (float)r8[4 + e];
        }
      }
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        v[k].set(e, a[e]);
        v[k].set(4 + e, b[e]);
      }
      v[k].store(Y + m * p.ldy + c);
    }
  }
  if (t == 0) shift_s = v[0].get(0);  // element (row 0, first channel of the group) of the rounded tensor: gn_small_kernel's shift
  __syncthreads();
  const float shift = shift_s;
  float s1 = 0.f, s2 = 0.f;
#pragma unroll
  for (int k = 0; k < VPT; ++k) {
    if (t + 256 * k < total) {
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const float d = v[k].get(e) - shift;
        s1 += d;
        s2 += d * d;
      }
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    s1 += __shfl_xor(s1, o);
    s2 += __shfl_xor(s2, o);
  }
  if ((t & 63) == 0) {
    red[0][t >> 6] = s1;
    red[1][t >> 6] = s2;
  }
  __syncthreads();
  const double a = ((double)red[0][0] + (double)red[0][1]) + ((double)red[0][2] + (double)red[0][3]);
  const double b = ((double)red[1][0] + (double)red[1][1]) + ((double)red[1][2] + (double)red[1][3]);
  const double cnt = (double)HW * gs;
  const double md = a / cnt;
  double var = b / cnt - md * md;
  if (var < 0.0) var = 0.0;
  const float mean = (float)((double)shift + md);
  const float rstd = (float)(1.0 / sqrt(var + (double)p.gn_eps));
  bf16* yb = reinterpret_cast<bf16*>(p.gn_y) + (long)n * HW * C + c_beg;
#pragma unroll
  for (int k = 0; k < VPT; ++k) {
    if (t + 256 * k < total) {
      const int c = c_beg + cv[k] * 8;
      const f32x4 g0 = *reinterpret_cast<const f32x4*>(p.gn_gamma + c), g1 = *reinterpret_cast<const f32x4*>(p.gn_gamma + c + 4);
      const f32x4 b0 = *reinterpret_cast<const f32x4*>(p.gn_beta + c), b1 = *reinterpret_cast<const f32x4*>(p.gn_beta + c + 4);
      crg_vec8<bf16> o;
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        const float ga = e < 4 ? g0[e] : g1[e - 4], be = e < 4 ? b0[e] : b1[e - 4];
        float f = (v[k].get(e) - mean) * (rstd * ga) + be;
        if (p.gn_silu) f = crg_silu_f(f);
        o.set(e, f);
      }
      o.store(yb + (long)row[k] * C + cv[k] * 8);
    }
  }
}

}  // namespace

namespace crg_mm {
// the reduce launch behind a split-K launch (whole problem, or - tail split - the rows >= slab_row0)
int launch_reduce(crg_ctx* ctx, hipStream_t st, const GemmP& p, const crg_plan::Plan& pl, int batch, bool y_f32) {
  const long rows = p.M - p.slab_row0;
  crg_prof_scope ps(ctx, st, CRG_K_SPLITK, (double)batch * p.splits * rows * p.N, (double)batch * rows * p.N * (4.0 * p.splits + (y_f32 ? 4 : 2)));
  const dim3 grid(pl.reduce_gx, pl.reduce_gy);
  KernFn kern = nullptr;
  switch (pl.reduce) {
    case CRG_REDUCE_GN:
      switch (pl.reduce_vpt) {
        case 1: kern = splitk_reduce_gn_kernel<1>; break;
        case 2: kern = splitk_reduce_gn_kernel<2>; break;
        case 3: kern = splitk_reduce_gn_kernel<3>; break;
        case 4: kern = splitk_reduce_gn_kernel<4>; break;
        case 5: kern = splitk_reduce_gn_kernel<5>; break;
        case 6: kern = splitk_reduce_gn_kernel<6>; break;
        default: kern = splitk_reduce_gn_kernel<8>; break;
      }
      break;
    case CRG_REDUCE_ROWS: kern = splitk_reduce_rows_kernel; break;
    case CRG_REDUCE_STATS: kern = y_f32 ? splitk_reduce_stats_kernel<float> : splitk_reduce_stats_kernel<bf16>; break;
    default: kern = y_f32 ? splitk_reduce_kernel<float> : splitk_reduce_kernel<bf16>; break;
  }
  hipLaunchKernelGGL(kern, grid, dim3(256), 0, st, p);
  CRG_CHECK_LAUNCH(ctx, pl.reduce == CRG_REDUCE_GN ? "splitk_reduce_gn" : "splitk_reduce");
  return 0;
}
}  // namespace crg_mm
