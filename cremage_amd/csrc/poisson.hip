// Gradient-domain (Poisson) paste of a rectangle: crg_poisson_clone (include/crg_hip.h).  The five-point system on the patch
// rectangle inset by 2 is solved directly by the type-I sine transform, u = S_n ((S_n F S_m) * rden) S_m, as four batched fp32
// products on v_mfma_f32_32x32x2_f32 (exact fp32: a k-ordered fmaf chain).  No half type anywhere: the bf16 and the fp16 build of the
// library compile this file to the same code.
#include "crg_common.h"

namespace {
inline int pc_grid_for(long n) {
  long g = (n + 255) / 256;
  return (int)(g < 1 ? 1 : (g > 65535 ? 65535 : g));
}

// F = L with the ring values moved to the right-hand side, one thread per interior pixel (i, j) of one (image, channel) plane; region
// coordinates are r = i + 1, c = j + 1 in the patch rectangle inset by 1 (hp x wp).  Integer arithmetic: |F| <= 8 * 255, exact in fp32.
__global__ __launch_bounds__(256) void poisson_rhs_kernel(const crg_poisson_args a, float* __restrict__ F, long total) {
  const int n = a.h - 4, m = a.w - 4, hp = a.h - 2, wp = a.w - 2, mg = a.margin;
  for (long idx = (long)blockIdx.x * 256 + threadIdx.x; idx < total; idx += (long)gridDim.x * 256) {
    const int j = (int)(idx % m);
    const long t = idx / m;
    const int i = (int)(t % n);
    const long plane = t / n;
    const unsigned char* d = (const unsigned char*)a.image + (plane / 3) * a.img_sn + (plane % 3) * a.img_sc + (long)(a.y + 1) * a.img_sy +
                             (long)(a.x + 1) * a.img_sx;
    const unsigned char* s = (const unsigned char*)a.patch + (plane / 3) * a.pat_sn + (plane % 3) * a.pat_sc + a.pat_sy + a.pat_sx;
    const int r = i + 1, c = j + 1;  // 1 <= r <= hp - 2, 1 <= c <= wp - 2: every read below stays inside the region
    auto D = [&](int rr, int cc) { return (int)d[rr * a.img_sy + cc * a.img_sx]; };
    auto S = [&](int rr, int cc) { return (int)s[rr * a.pat_sy + cc * a.pat_sx]; };
    auto in_mask = [&](int rr, int cc) { return rr >= mg && rr < hp - mg && cc >= mg && cc < wp - mg; };
    auto vx = [&](int rr, int cc) { return in_mask(rr, cc) ? S(rr, cc + 1) - S(rr, cc) : D(rr, cc + 1) - D(rr, cc); };
    auto vy = [&](int rr, int cc) { return in_mask(rr, cc) ? S(rr + 1, cc) - S(rr, cc) : D(rr + 1, cc) - D(rr, cc); };
    int v = vx(r, c) - vx(r, c - 1) + vy(r, c) - vy(r - 1, c);
    if (r == 1) v -= D(0, c);
    if (r == hp - 2) v -= D(hp - 1, c);
    if (c == 1) v -= D(r, 0);
    if (c == wp - 2) v -= D(r, wp - 1);
    F[idx] = (float)v;
  }
}

// C[b] = A[b] * B[b], row-major fp32, M, N and K ragged; a batch stride of 0 shares the operand (the sine matrix).  One block: 64 x 64
// of C, four waves of one 32 x 32 accumulator each, K in steps of 32 through LDS.  Lane l of v_mfma_f32_32x32x2_f32 supplies
// A[i = l & 31][k = l >> 5] and B[k = l >> 5][j = l & 31], so both tiles lie k-major in LDS and a half-wave reads 32 consecutive words.
// The A tile is stored transposed: its row stride of 65 words spreads the 32 k of a row, which one half-wave writes, over the banks.
// Loads past M, N or K read the clamped (valid) address and count as 0; stores past M or N do not happen.
constexpr int PG_T = 64, PG_BK = 32, PG_LDA = PG_T + 1;
enum { PG_PLAIN = 0, PG_SCALE = 1, PG_FINAL = 2 };

struct pg_args {
  const float* A;
  long lda, a_bs;
  const float* B;
  long ldb, b_bs;
  float* C;  // PG_FINAL: the optional field
  long ldc, c_bs;
  int M, N, K;
  const float* scale;  // PG_SCALE: [M][N]
  unsigned char* img;  // PG_FINAL: pixel (0, 0) of the interior in plane 0 of image 0
  long i_sn, i_sc, i_sy, i_sx;
};

template <int EPI>
__global__ __launch_bounds__(256) void poisson_gemm_kernel(const pg_args a) {
  __shared__ float As[PG_BK * PG_LDA];
  __shared__ float Bs[PG_BK * PG_T];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave >> 1, wn = wave & 1;
  const int m0 = blockIdx.y * PG_T, n0 = blockIdx.x * PG_T;
  const long b = blockIdx.z;
  const float* A = a.A + b * a.a_bs;
  const float* B = a.B + b * a.b_bs;
  f32x16 acc;
#pragma unroll
  for (int e = 0; e < 16; ++e) acc[e] = 0.f;
  const int ak = tid & 31, ar = tid >> 5;  // A: k ak of rows ar, ar + 8, ...
  const int bc = tid & 63, bk = tid >> 6;  // B: column bc of k bk, bk + 4, ...
  const int gn = n0 + bc;
  for (int k0 = 0; k0 < a.K; k0 += PG_BK) {
    {
      const int gk = k0 + ak;
#pragma unroll
      for (int i = 0; i < PG_T / 8; ++i) {
        const int row = ar + 8 * i, gm = m0 + row;
        const float v = A[(long)min(gm, a.M - 1) * a.lda + min(gk, a.K - 1)];
        As[ak * PG_LDA + row] = (gm < a.M && gk < a.K) ? v : 0.f;
      }
    }
#pragma unroll
    for (int i = 0; i < PG_BK / 4; ++i) {
      const int k = bk + 4 * i, gk = k0 + k;
      const float v = B[(long)min(gk, a.K - 1) * a.ldb + min(gn, a.N - 1)];
      Bs[k * PG_T + bc] = (gk < a.K && gn < a.N) ? v : 0.f;
    }
    __syncthreads();
#pragma unroll
    for (int kk = 0; kk < PG_BK; kk += 2) {
      const float av = As[(kk + (lane >> 5)) * PG_LDA + wm * 32 + (lane & 31)];
      const float bv = Bs[(kk + (lane >> 5)) * PG_T + wn * 32 + (lane & 31)];
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bv, acc, 0, 0, 0);
    }
    __syncthreads();
  }
  // C/D: column = lane & 31, row = (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5)
  const int col = n0 + wn * 32 + (lane & 31);
  if (col >= a.N) return;
#pragma unroll
  for (int e = 0; e < 16; ++e) {
    const int row = m0 + wm * 32 + (e & 3) + 8 * (e >> 2) + 4 * (lane >> 5);
    if (row >= a.M) continue;
    float v = acc[e];
    if (EPI == PG_SCALE) v *= a.scale[(long)row * a.N + col];
    if (EPI == PG_FINAL) {
      if (a.C) a.C[b * a.c_bs + (long)row * a.ldc + col] = v;
      const float q = fminf(fmaxf(rintf(v), 0.f), 255.f);  // v_rndne_f32: half to even
      a.img[(b / 3) * a.i_sn + (b % 3) * a.i_sc + (long)row * a.i_sy + (long)col * a.i_sx] = (unsigned char)(int)q;
    } else {
      a.C[b * a.c_bs + (long)row * a.ldc + col] = v;
    }
  }
}

template <int EPI>
void pg_launch(const pg_args& g, int batch, hipStream_t st) {
  const dim3 grid((g.N + PG_T - 1) / PG_T, (g.M + PG_T - 1) / PG_T, batch);
  hipLaunchKernelGGL((poisson_gemm_kernel<EPI>), grid, dim3(256), 0, st, g);
}
}  // namespace

extern "C" int crg_poisson_clone(crg_ctx* ctx, void* stream, const crg_poisson_args* args) {
  if (!ctx) return -22;
  CRG_REQUIRE(ctx, args != nullptr, "poisson_clone: null args");
  const crg_poisson_args& a = *args;
  CRG_REQUIRE(ctx, a.image && a.patch, "poisson_clone: null image or patch");
  CRG_REQUIRE(ctx, a.s_rows && a.s_cols && a.rden && a.work, "poisson_clone: null table or workspace");
  CRG_REQUIRE(ctx, a.N > 0 && (int64_t)a.N * 3 <= 65535, "poisson_clone: N = %d must be in 1..21845", a.N);
  CRG_REQUIRE(ctx, a.h >= 5 && a.w >= 5, "poisson_clone: a %dx%d patch has no interior", a.h, a.w);
  CRG_REQUIRE(ctx, a.margin >= 0, "poisson_clone: margin %d is negative", a.margin);
  CRG_REQUIRE(ctx, a.img_h > 0 && a.img_w > 0 && a.x >= 0 && a.y >= 0 && a.x <= a.img_w - a.w && a.y <= a.img_h - a.h,
              "poisson_clone: patch %dx%d at (x %d, y %d) lies outside the %dx%d image", a.h, a.w, a.x, a.y, a.img_h, a.img_w);
  CRG_REQUIRE(ctx, a.img_sx > 0 && a.img_sy > 0 && a.img_sc > 0 && (a.img_sn > 0 || a.N == 1) && a.img_sn >= 0,
              "poisson_clone: image strides must be positive");
  CRG_REQUIRE(ctx, a.pat_sx > 0 && a.pat_sy > 0 && a.pat_sc >= 0 && a.pat_sn >= 0, "poisson_clone: patch strides must be positive (n and c: not negative)");
  const int n = a.h - 4, m = a.w - 4;
  CRG_REQUIRE(ctx, (n + PG_T - 1) / PG_T <= 65535, "poisson_clone: patch %dx%d is too large", a.h, a.w);
  // byte intervals: the image rectangle (read and written) and the patch (read)
  const char* i0 = (const char*)a.image + a.y * a.img_sy + a.x * a.img_sx;
  const char* i1 = i0 + (a.N - 1) * a.img_sn + 2 * a.img_sc + (a.h - 1) * a.img_sy + (a.w - 1) * a.img_sx + 1;
  const char* p0 = (const char*)a.patch;
  const char* p1 = p0 + (a.N - 1) * a.pat_sn + 2 * a.pat_sc + (a.h - 1) * a.pat_sy + (a.w - 1) * a.pat_sx + 1;
  CRG_REQUIRE(ctx, i1 <= p0 || p1 <= i0, "poisson_clone: image and patch overlap");
  hipStream_t st = (hipStream_t)stream;
  const int batch = a.N * 3;
  const long plane = (long)n * m, total = plane * batch;
  float* w0 = a.work;
  float* w1 = a.work + total;
  // one profiling record for the call (the slot table has no fp32-GEMM row): the four products' FLOPs, the passes' traffic
  crg_prof_scope ps(ctx, st, CRG_K_ELEMENTWISE, 4.0 * total * (n + m), 4.0 * total * 9.0 + 8.0 * ((double)n * n + (double)m * m));
  hipLaunchKernelGGL(poisson_rhs_kernel, dim3(pc_grid_for(total)), dim3(256), 0, st, a, w0, total);
  CRG_CHECK_LAUNCH(ctx, "poisson_clone (right-hand side)");
  pg_args g = {};
  g.M = n;
  g.N = m;
  g.ldc = m;
  g.c_bs = plane;
  // w1 = S_n w0
  g.A = a.s_rows, g.lda = n, g.a_bs = 0, g.B = w0, g.ldb = m, g.b_bs = plane, g.C = w1, g.K = n;
  pg_launch<PG_PLAIN>(g, batch, st);
  CRG_CHECK_LAUNCH(ctx, "poisson_clone (S_n F)");
  // w0 = (w1 S_m) * rden
  g.A = w1, g.lda = m, g.a_bs = plane, g.B = a.s_cols, g.ldb = m, g.b_bs = 0, g.C = w0, g.K = m, g.scale = a.rden;
  pg_launch<PG_SCALE>(g, batch, st);
  CRG_CHECK_LAUNCH(ctx, "poisson_clone (S_n F S_m)");
  // w1 = S_n w0
  g.A = a.s_rows, g.lda = n, g.a_bs = 0, g.B = w0, g.ldb = m, g.b_bs = plane, g.C = w1, g.K = n, g.scale = nullptr;
  pg_launch<PG_PLAIN>(g, batch, st);
  CRG_CHECK_LAUNCH(ctx, "poisson_clone (S_n T)");
  // image interior = clip(rint(w1 S_m)), field = w1 S_m
  g.A = w1, g.lda = m, g.a_bs = plane, g.B = a.s_cols, g.ldb = m, g.b_bs = 0, g.C = a.field, g.K = m;
  g.img = (unsigned char*)a.image + (long)(a.y + 2) * a.img_sy + (long)(a.x + 2) * a.img_sx;
  g.i_sn = a.img_sn, g.i_sc = a.img_sc, g.i_sy = a.img_sy, g.i_sx = a.img_sx;
  pg_launch<PG_FINAL>(g, batch, st);
  CRG_CHECK_LAUNCH(ctx, "poisson_clone (S_n T S_m)");
  return 0;
}
