// The blurred-mask composite of inpainting and spot inpainting: crg_blur_blend_u8 (include/crg_hip.h), one launch.  The definition is
// cremage_amd.postprocess.blend_blurred_mask (numpy: float64 separable 11 x 11 Gaussian, fp32 blend) and the bytes are equal, so NOTHING
// in this file may contract a multiply and an add: numpy never does, hipcc does by default.  No half type anywhere: the bf16 and the
// fp16 build of the library compile this file to the same code.
#include "crg_common.h"

#pragma clang fp contract(off)  // file scope: every function below

namespace {
// One block: a BB_TX x BB_TY tile of pixels of one image, 256 threads.  LDS: the tile's grey bytes with a halo of 5 (42 x 74, row pitch
// 76) and the horizontal pass over all 42 rows as doubles (42 x 64): 3192 + 21504 bytes, six blocks per CU by LDS.  A lane reads and
// writes column `lane` of a row of doubles: 32 consecutive 8-byte words per half-wave, every bank once.  The vertical pass keeps the 18
// doubles of a thread's 8 rows in registers.  The horizontal pass runs over 42 rows for 32 of output: 1.31 x the minimum.
constexpr int BB_TX = 64, BB_TY = 32, BB_R = 5;
constexpr int BB_GH = BB_TY + 2 * BB_R, BB_GW = BB_TX + 2 * BB_R, BB_GP = 76;
constexpr int BB_ROWS = BB_TY / 4;  // rows per thread in the vertical pass

// BORDER_REFLECT_101 for -5 <= i <= n + 4 with n >= 6; anything further out (the part of a ragged tile past the image plus its halo,
// whose results are never stored) is clamped into the image.
__device__ __forceinline__ int bb_refl(int i, int n) {
  if (i < 0) i = -i;
  if (i >= n) i = 2 * n - 2 - i;
  return min(max(i, 0), n - 1);
}

template <int GRAY>
__global__ __launch_bounds__(256) void blur_blend_kernel(const crg_blend_args a) {
  __shared__ unsigned char g8[BB_GH * BB_GP];
  __shared__ double hrow[BB_GH * BB_TX];
  const int tid = threadIdx.x;
  const int cx = tid & (BB_TX - 1), ry = tid >> 6;
  const int X0 = blockIdx.x * BB_TX, Y0 = blockIdx.y * BB_TY;
  const long n = blockIdx.z;
  const unsigned char* org = (const unsigned char*)a.original + n * a.org_sn;
  const unsigned char* upd = (const unsigned char*)a.updated + n * a.upd_sn;
  const unsigned char* msk = (const unsigned char*)a.mask + n * a.msk_sn;
  unsigned char* out = (unsigned char*)a.out + n * a.out_sn;
  const int x = X0 + cx;
  if (a.win_w > 0 && (X0 >= a.win_x + a.win_w || X0 + BB_TX <= a.win_x || Y0 >= a.win_y + a.win_h || Y0 + BB_TY <= a.win_y)) {
    // the whole tile lies outside the window (block-uniform): m = 0 there and the result is the original byte
    if ((const void*)out == (const void*)org || x >= a.W) return;
#pragma unroll
    for (int r = 0; r < BB_ROWS; ++r) {
      const int y = Y0 + ry * BB_ROWS + r;
      if (y >= a.H) break;
      const unsigned char* o = org + (long)y * a.org_sy + (long)x * a.org_sx;
      unsigned char* d = out + (long)y * a.out_sy + (long)x * a.out_sx;
      for (int c = 0; c < a.C; ++c) d[c] = o[c];
    }
    return;
  }
  // grey bytes of the tile and its halo, reflected at the image's borders
  for (int i = tid; i < BB_GH * BB_GW; i += 256) {
    const int r = i / BB_GW, c = i - r * BB_GW;
    const int gy = bb_refl(Y0 - BB_R + r, a.H), gx = bb_refl(X0 - BB_R + c, a.W);
    const unsigned char* p = msk + (long)gy * a.msk_sy + (long)gx * a.msk_sx;
    int g = p[0];
    if (GRAY) g = (g * 4899 + (int)p[1] * 9617 + (int)p[2] * 1868 + 8192) >> 14;
    g8[r * BB_GP + c] = (unsigned char)g;
  }
  __syncthreads();
  // horizontal pass over every row, the halo rows included: column cx of rows ry, ry + 4, ...
  for (int r = ry; r < BB_GH; r += 4) {
    const unsigned char* row = g8 + r * BB_GP + cx;
    double s = a.taps[0] * (double)row[0];
#pragma unroll
    for (int i = 1; i < 11; ++i) s = s + a.taps[i] * (double)row[i];
    hrow[r * BB_TX + cx] = s;
  }
  __syncthreads();
  // vertical pass, rounding and blend: column cx of rows BB_ROWS * ry .. + BB_ROWS - 1
  double hv[BB_ROWS + 2 * BB_R];
#pragma unroll
  for (int i = 0; i < BB_ROWS + 2 * BB_R; ++i) hv[i] = hrow[(ry * BB_ROWS + i) * BB_TX + cx];
  if (x >= a.W) return;
#pragma unroll
  for (int r = 0; r < BB_ROWS; ++r) {
    const int y = Y0 + ry * BB_ROWS + r;
    if (y >= a.H) break;
    double s = a.taps[0] * hv[r];
#pragma unroll
    for (int i = 1; i < 11; ++i) s = s + a.taps[i] * hv[r + i];
    const double q = fmin(fmax(floor(s + 0.5), 0.0), 255.0);
    const float m = (float)(int)q / 255.0f;
    const float t = 1.0f - m;
    const unsigned char* o = org + (long)y * a.org_sy + (long)x * a.org_sx;
    const unsigned char* u = upd + (long)y * a.upd_sy + (long)x * a.upd_sx;
    unsigned char* d = out + (long)y * a.out_sy + (long)x * a.out_sx;
    for (int c = 0; c < a.C; ++c) {
      const float pu = (float)u[c] * m;
      const float po = (float)o[c] * t;
      const float v = fminf(fmaxf(pu + po, 0.f), 255.f);
      d[c] = (unsigned char)(int)v;
    }
  }
}

// [first, last) bytes of a strided [N][H][W][ch] uint8 image
inline void bb_extent(const void* p, const crg_blend_args& a, int64_t sn, int64_t sy, int64_t sx, int ch, const char** lo, const char** hi) {
  *lo = (const char*)p;
  *hi = *lo + (a.N - 1) * sn + (a.H - 1) * sy + (a.W - 1) * sx + ch;
}
}  // namespace

extern "C" int crg_blur_blend_u8(crg_ctx* ctx, void* stream, const crg_blend_args* args) {
  if (!ctx) return -22;
  CRG_REQUIRE(ctx, args != nullptr, "blur_blend_u8: null args");
  const crg_blend_args& a = *args;
  CRG_REQUIRE(ctx, a.original && a.updated && a.mask && a.out, "blur_blend_u8: null image, mask or destination");
  CRG_REQUIRE(ctx, a.N > 0 && a.N <= 65535, "blur_blend_u8: N = %d must be in 1..65535", a.N);
  CRG_REQUIRE(ctx, a.H >= 6 && a.W >= 6, "blur_blend_u8: a %dx%d image is smaller than 6x6 (radius-5 reflect-101 border)", a.H, a.W);
  CRG_REQUIRE(ctx, (a.H + BB_TY - 1) / BB_TY <= 65535, "blur_blend_u8: image %dx%d is too large", a.H, a.W);
  CRG_REQUIRE(ctx, a.C >= 1 && a.C <= 4, "blur_blend_u8: C = %d must be in 1..4", a.C);
  CRG_REQUIRE(ctx, a.gray_mode == 0 || a.gray_mode == 1, "blur_blend_u8: gray_mode %d must be 0 or 1", a.gray_mode);
  const int mch = a.gray_mode ? 3 : 1;
  CRG_REQUIRE(ctx, a.org_sx >= a.C && a.upd_sx >= a.C && a.out_sx >= a.C && a.msk_sx >= mch, "blur_blend_u8: a pixel stride is smaller than the pixel");
  CRG_REQUIRE(ctx, a.org_sy > 0 && a.upd_sy > 0 && a.out_sy > 0 && a.msk_sy > 0, "blur_blend_u8: row strides must be positive");
  CRG_REQUIRE(ctx, a.org_sn >= 0 && a.upd_sn >= 0 && a.msk_sn >= 0 && (a.out_sn > 0 || a.N == 1) && a.out_sn >= 0,
              "blur_blend_u8: image strides must not be negative (destination: positive)");
  CRG_REQUIRE(ctx, a.win_w >= 0 && a.win_h >= 0 && (a.win_w == 0) == (a.win_h == 0), "blur_blend_u8: window %dx%d is malformed", a.win_w, a.win_h);
  if (a.win_w > 0)
    CRG_REQUIRE(ctx, a.win_x >= 0 && a.win_y >= 0 && a.win_x <= a.W - a.win_w && a.win_y <= a.H - a.win_h,
                "blur_blend_u8: window (x %d, y %d, w %d, h %d) lies outside the %dx%d image", a.win_x, a.win_y, a.win_w, a.win_h, a.H, a.W);
  for (int i = 0; i < 11; ++i) CRG_REQUIRE(ctx, a.taps[i] == a.taps[i] && a.taps[i] >= 0.0 && a.taps[i] <= 1.0, "blur_blend_u8: tap %d is not in [0, 1]", i);
  const char *o0, *o1, *u0, *u1, *m0, *m1, *d0, *d1;
  bb_extent(a.original, a, a.org_sn, a.org_sy, a.org_sx, a.C, &o0, &o1);
  bb_extent(a.updated, a, a.upd_sn, a.upd_sy, a.upd_sx, a.C, &u0, &u1);
  bb_extent(a.mask, a, a.msk_sn, a.msk_sy, a.msk_sx, mch, &m0, &m1);
  bb_extent(a.out, a, a.out_sn, a.out_sy, a.out_sx, a.C, &d0, &d1);
  CRG_REQUIRE(ctx, (d1 <= u0 || u1 <= d0) && (d1 <= m0 || m1 <= d0), "blur_blend_u8: the destination overlaps the updated image or the mask");
  const bool inplace = a.out == a.original;
  if (inplace)
    CRG_REQUIRE(ctx, a.out_sn == a.org_sn && a.out_sy == a.org_sy && a.out_sx == a.org_sx, "blur_blend_u8: in place needs the original's strides");
  else
    CRG_REQUIRE(ctx, d1 <= o0 || o1 <= d0, "blur_blend_u8: the destination overlaps the original without being it");
  hipStream_t st = (hipStream_t)stream;
  const double px = (double)a.N * (a.win_w > 0 ? (double)a.win_w * a.win_h : (double)a.H * a.W);
  crg_prof_scope ps(ctx, st, CRG_K_ELEMENTWISE, px * (2.0 * 21.0 * (1.0 + (double)BB_GH / BB_TY) + 6.0 + 5.0 * a.C), px * (mch + 3.0 * a.C));
  const dim3 grid((a.W + BB_TX - 1) / BB_TX, (a.H + BB_TY - 1) / BB_TY, a.N);
  if (a.gray_mode) hipLaunchKernelGGL(blur_blend_kernel<1>, grid, dim3(256), 0, st, a);
  else hipLaunchKernelGGL(blur_blend_kernel<0>, grid, dim3(256), 0, st, a);
  CRG_CHECK_LAUNCH(ctx, "blur_blend_u8");
  return 0;
}
