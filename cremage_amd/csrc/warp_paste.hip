// The glue of face unblur / colorize on the device: crg_warp_affine_u8 and crg_paste_warped_u8 (include/crg_hip.h).  The definitions are
// cremage_amd.postprocess.warp_affine_tables / warp_affine_u8 / erode5_mask / paste_warped_face / _unit_to_face (numpy: float64 tables,
// int64 positions, integer weights) and the bytes are equal, so NOTHING in this file may contract a multiply and an add: numpy never does,
// hipcc does by default.  No half type anywhere: the bf16 and the fp16 build of the library compile this file to the same code.
#include <math.h>

#include "crg_common.h"

#pragma clang fp contract(off)  // file scope: every function below

namespace {
constexpr int WP_MAPS = 16;  // destination-to-source maps per launch: 768 bytes of kernel arguments

struct wp_map {
  double m00, m01, m02, m10, m11, m12;
};
struct wp_maps {
  wp_map m[WP_MAPS];
};
// the image a warp reads: uint8 [h][w][C] (sc = 1) or fp32 [C][h][w]; strides in elements
struct wp_src {
  const void* p;
  long sc, sy, sx;
  int h, w, C;
};

// warp_affine_tables' cut: rint (half to even), clipped to +- 2^40, as int64
__device__ __forceinline__ long wp_cut(double v) { return (long)fmin(fmax(rint(v), -0x1p40), 0x1p40); }

// one source element as a byte; fp32 is quantised as _unit_to_face does: clamp(0, 1), one fp32 product, truncation
template <bool F32>
__device__ __forceinline__ int wp_tap(const void* p, long off) {
  if (F32) return (int)(fminf(fmaxf(((const float*)p)[off], 0.f), 1.f) * 255.0f);
  return ((const unsigned char*)p)[off];
}

// warp_affine_u8 at destination pixel (x, y): the table entries of column x and row y are formed here, in the tables' operation order;
// positions stay 64-bit until after the inside test (a neighbour outside the source counts 0 and is never addressed)
template <bool F32>
__device__ __forceinline__ void wp_sample(const wp_src& s, const wp_map& m, int x, int y, int (&out)[4]) {
  const double xs = (double)x, ys = (double)y;
  const long ax = wp_cut(m.m00 * xs * 1024.0), bx = wp_cut(m.m10 * xs * 1024.0);
  const long x0 = wp_cut((m.m01 * ys + m.m02) * 1024.0) + 16, y0 = wp_cut((m.m11 * ys + m.m12) * 1024.0) + 16;
  const long X = (x0 + ax) >> 5, Y = (y0 + bx) >> 5;  // 1 / 32 pixel; arithmetic shifts
  const long sx = X >> 5, sy = Y >> 5;
  const int fx = (int)(X & 31), fy = (int)(Y & 31);
  int acc[4] = {0, 0, 0, 0};
#pragma unroll
  for (int dy = 0; dy < 2; ++dy) {
#pragma unroll
    for (int dx = 0; dx < 2; ++dx) {
      const long px = sx + dx, py = sy + dy;
      if (px < 0 || px >= s.w || py < 0 || py >= s.h) continue;
      const int wgt = (dx ? fx : 32 - fx) * (dy ? fy : 32 - fy) * 32;
      const long off = py * s.sy + px * s.sx;
#pragma unroll
      for (int c = 0; c < 4; ++c)
        if (c < s.C) acc[c] += wgt * wp_tap<F32>(s.p, off + c * s.sc);
    }
  }
#pragma unroll
  for (int c = 0; c < 4; ++c) out[c] = (acc[c] + (1 << 14)) >> 15;
}

// One thread per destination pixel, a block 64 x 4 pixels of image n0 + blockIdx.z.  The destination is uint8 [N][H][W][C] (strides in bytes)
// or fp32 [N][C][H][W] (strides in elements) holding byte / 255.0f, the division correctly rounded.
template <bool DST_F32>
__global__ __launch_bounds__(256) void warp_affine_kernel(const wp_src s, const wp_maps maps, void* dst, long dn, long dc, long dy, long dx, int H,
                                                          int W, int n0) {
  const int x = blockIdx.x * 64 + (threadIdx.x & 63), y = blockIdx.y * 4 + (threadIdx.x >> 6);
  if (x >= W || y >= H) return;
  int v[4];
  wp_sample<false>(s, maps.m[blockIdx.z], x, y, v);
  const long base = (long)(n0 + blockIdx.z) * dn + (long)y * dy + (long)x * dx;
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    if (c >= s.C) break;
    if (DST_F32) ((float*)dst)[base + c * dc] = (float)v[c] / 255.0f;
    else ((unsigned char*)dst)[base + c] = (unsigned char)v[c];
  }
}

// One block: a PW_TX x PW_TY tile of image pixels, 256 threads.  LDS: the warped pixels of the tile and a halo of 2, a pixel's C bytes in one
// word (the bytes of absent channels and of pixels outside the image are 0xff: set, they do not constrain), and the horizontal AND of
// the mask over all 20 rows: 5440 + 5120 bytes.  Consecutive lanes read consecutive words.  Five horizontal and five vertical ANDs of a
// word that carries one mask byte per channel.  A thread stores the bytes of its own pixels, one by one; the image is never read.
constexpr int PW_TX = 64, PW_TY = 16, PW_R = 2;
constexpr int PW_GW = PW_TX + 2 * PW_R, PW_GH = PW_TY + 2 * PW_R;
constexpr int PW_ROWS = PW_TY / 4;  // rows per thread in the vertical pass

// 0xff in every byte of m that is not zero
__device__ __forceinline__ unsigned pw_mask(unsigned v) {
  unsigned m = 0;
#pragma unroll
  for (int c = 0; c < 4; ++c)
    if ((v >> (8 * c)) & 0xffu) m |= 0xffu << (8 * c);
  return m;
}

template <bool F32>
__global__ __launch_bounds__(256) void paste_warped_kernel(const wp_src s, const wp_map m, unsigned char* image, long isy, long isx, int H, int W,
                                                           int tile_x0, int tile_y0) {
  __shared__ unsigned warped[PW_GH * PW_GW];
  __shared__ unsigned hand[PW_GH * PW_TX];
  const int tid = threadIdx.x;
  const int X0 = (tile_x0 + (int)blockIdx.x) * PW_TX, Y0 = (tile_y0 + (int)blockIdx.y) * PW_TY;
  for (int i = tid; i < PW_GH * PW_GW; i += 256) {
    const int r = i / PW_GW, c = i - r * PW_GW;
    const int gx = X0 - PW_R + c, gy = Y0 - PW_R + r;
    unsigned word = 0xffffffffu;
    if (gx >= 0 && gx < W && gy >= 0 && gy < H) {
      int v[4];
      wp_sample<F32>(s, m, gx, gy, v);
#pragma unroll
      for (int ch = 0; ch < 4; ++ch)
        if (ch < s.C) word = (word & ~(0xffu << (8 * ch))) | ((unsigned)v[ch] << (8 * ch));
    }
    warped[i] = word;
  }
  __syncthreads();
  const int cx = tid & (PW_TX - 1), ry = tid >> 6;
  for (int r = ry; r < PW_GH; r += 4) {
    const unsigned* row = warped + r * PW_GW + cx;
    unsigned a = pw_mask(row[0]);
#pragma unroll
    for (int i = 1; i < 2 * PW_R + 1; ++i) a &= pw_mask(row[i]);
    hand[r * PW_TX + cx] = a;
  }
  __syncthreads();
  const int x = X0 + cx;
  if (x >= W) return;
#pragma unroll
  for (int r = 0; r < PW_ROWS; ++r) {
    const int ty = ry * PW_ROWS + r, y = Y0 + ty;
    if (y >= H) break;
    unsigned a = hand[ty * PW_TX + cx];
#pragma unroll
    for (int i = 1; i < 2 * PW_R + 1; ++i) a &= hand[(ty + i) * PW_TX + cx];
    const unsigned v = warped[(ty + PW_R) * PW_GW + cx + PW_R];
    unsigned char* d = image + (long)y * isy + (long)x * isx;
#pragma unroll
    for (int ch = 0; ch < 4; ++ch)
      if (ch < s.C && ((a >> (8 * ch)) & 1u)) d[ch] = (unsigned char)(v >> (8 * ch));
  }
}

inline bool wp_finite(const double* m, int count) {
  for (int i = 0; i < count; ++i)
    if (!std::isfinite(m[i])) return false;
  return true;
}
inline wp_map wp_load(const double* m) { return wp_map{m[0], m[1], m[2], m[3], m[4], m[5]}; }
}  // namespace

extern "C" int crg_warp_affine_u8(crg_ctx* ctx, void* stream, const void* src, int64_t src_sy, int64_t src_sx, int h, int w, int C,
                                  const double* dst_to_src, int N, void* dst, int dst_f32, int64_t dst_sn, int64_t dst_sc, int64_t dst_sy,
                                  int64_t dst_sx, int H, int W) {
  if (!ctx) return -22;
  CRG_REQUIRE(ctx, src && dst && dst_to_src, "warp_affine_u8: null source, destination or maps");
  CRG_REQUIRE(ctx, C >= 1 && C <= 4, "warp_affine_u8: C = %d must be in 1..4", C);
  CRG_REQUIRE(ctx, h >= 1 && w >= 1 && H >= 1 && W >= 1 && N >= 1, "warp_affine_u8: empty size (source %dx%d, %d destinations of %dx%d)", h, w, N, H, W);
  CRG_REQUIRE(ctx, (H + 3) / 4 <= 65535 && N <= (1 << 20), "warp_affine_u8: %d destinations of %dx%d are too large", N, H, W);
  CRG_REQUIRE(ctx, dst_f32 == 0 || dst_f32 == 1, "warp_affine_u8: dst_f32 = %d must be 0 or 1", dst_f32);
  CRG_REQUIRE(ctx, src_sy >= 0 && src_sx >= 0 && dst_sn >= 0 && dst_sc >= 0 && dst_sy >= 0 && dst_sx >= 0, "warp_affine_u8: strides must not be negative");
  CRG_REQUIRE(ctx, src_sx >= C || w == 1, "warp_affine_u8: the channels of a source pixel must be adjacent (pixel stride %lld < C = %d)", (long long)src_sx, C);
  if (dst_f32)
    CRG_REQUIRE(ctx, (dst_sc > 0 || C == 1) && (dst_sy > 0 || H == 1) && (dst_sx > 0 || W == 1) && (dst_sn > 0 || N == 1),
                "warp_affine_u8: the strides of the fp32 destination must be positive");
  else
    CRG_REQUIRE(ctx, dst_sc == 1 && (dst_sx >= C || W == 1) && (dst_sy > 0 || H == 1) && (dst_sn > 0 || N == 1),
                "warp_affine_u8: the channels of a destination pixel must be adjacent and its strides positive");
  CRG_REQUIRE(ctx, wp_finite(dst_to_src, 6 * N), "warp_affine_u8: a coefficient is not finite");
  const int64_t esz = dst_f32 ? 4 : 1;
  const char *s0 = (const char*)src, *s1 = s0 + (h - 1) * src_sy + (w - 1) * src_sx + C;
  const char *d0 = (const char*)dst, *d1 = d0 + ((N - 1) * dst_sn + (C - 1) * dst_sc + (H - 1) * dst_sy + (W - 1) * dst_sx + 1) * esz;
  CRG_REQUIRE(ctx, d1 <= s0 || s1 <= d0, "warp_affine_u8: the destination overlaps the source");
  hipStream_t st = (hipStream_t)stream;
  const wp_src s{src, 1, src_sy, src_sx, h, w, C};
  for (int n0 = 0; n0 < N; n0 += WP_MAPS) {
    const int nb = N - n0 < WP_MAPS ? N - n0 : WP_MAPS;
    wp_maps maps = {};
    for (int i = 0; i < nb; ++i) maps.m[i] = wp_load(dst_to_src + 6 * (n0 + i));
    const double px = (double)nb * H * W;
    crg_prof_scope ps(ctx, st, CRG_K_ELEMENTWISE, px * (20.0 + 12.0 * C), px * C * (4.0 + esz));
    const dim3 grid((W + 63) / 64, (H + 3) / 4, nb);
    if (dst_f32) hipLaunchKernelGGL(warp_affine_kernel<true>, grid, dim3(256), 0, st, s, maps, dst, dst_sn, dst_sc, dst_sy, dst_sx, H, W, n0);
    else hipLaunchKernelGGL(warp_affine_kernel<false>, grid, dim3(256), 0, st, s, maps, dst, dst_sn, dst_sc, dst_sy, dst_sx, H, W, n0);
    CRG_CHECK_LAUNCH(ctx, "warp_affine_u8");
  }
  return 0;
}

extern "C" int crg_paste_warped_u8(crg_ctx* ctx, void* stream, void* image, int64_t img_sy, int64_t img_sx, int H, int W, int C, const void* face,
                                   int face_f32, int64_t face_sc, int64_t face_sy, int64_t face_sx, int h, int w, const double* face_from_image,
                                   int rect_x, int rect_y, int rect_w, int rect_h) {
  if (!ctx) return -22;
  CRG_REQUIRE(ctx, image && face && face_from_image, "paste_warped_u8: null image, face or map");
  CRG_REQUIRE(ctx, C >= 1 && C <= 4, "paste_warped_u8: C = %d must be in 1..4", C);
  CRG_REQUIRE(ctx, h >= 1 && w >= 1 && H >= 1 && W >= 1, "paste_warped_u8: empty size (face %dx%d, image %dx%d)", h, w, H, W);
  CRG_REQUIRE(ctx, face_f32 == 0 || face_f32 == 1, "paste_warped_u8: face_f32 = %d must be 0 or 1", face_f32);
  CRG_REQUIRE(ctx, img_sy >= 0 && img_sx >= 0 && face_sc >= 0 && face_sy >= 0 && face_sx >= 0, "paste_warped_u8: strides must not be negative");
  CRG_REQUIRE(ctx, (img_sx >= C || W == 1) && (img_sy > 0 || H == 1), "paste_warped_u8: the channels of an image pixel must be adjacent and its row stride positive");
  if (!face_f32)
    CRG_REQUIRE(ctx, face_sc == 1 && (face_sx >= C || w == 1), "paste_warped_u8: the channels of a uint8 face pixel must be adjacent");
  CRG_REQUIRE(ctx, wp_finite(face_from_image, 6), "paste_warped_u8: a coefficient is not finite");
  CRG_REQUIRE(ctx, rect_w >= 0 && rect_h >= 0 && rect_x >= 0 && rect_y >= 0 && rect_x <= W - rect_w && rect_y <= H - rect_h,
              "paste_warped_u8: rectangle (x %d, y %d, w %d, h %d) lies outside the %dx%d image", rect_x, rect_y, rect_w, rect_h, H, W);
  const int64_t esz = face_f32 ? 4 : 1;
  const char *i0 = (const char*)image, *i1 = i0 + (H - 1) * img_sy + (W - 1) * img_sx + C;
  const char *f0 = (const char*)face, *f1 = f0 + ((C - 1) * face_sc + (h - 1) * face_sy + (w - 1) * face_sx + 1) * esz;
  CRG_REQUIRE(ctx, i1 <= f0 || f1 <= i0, "paste_warped_u8: the image overlaps the face");
  if (rect_w == 0 || rect_h == 0) return 0;  // the caller states that nothing of the face reaches the image
  const int tx0 = rect_x / PW_TX, tx1 = (rect_x + rect_w - 1) / PW_TX, ty0 = rect_y / PW_TY, ty1 = (rect_y + rect_h - 1) / PW_TY;
  CRG_REQUIRE(ctx, ty1 - ty0 + 1 <= 65535, "paste_warped_u8: rectangle of %d rows is too large", rect_h);
  hipStream_t st = (hipStream_t)stream;
  const wp_src s{face, face_sc, face_sy, face_sx, h, w, C};
  const wp_map m = wp_load(face_from_image);
  const dim3 grid(tx1 - tx0 + 1, ty1 - ty0 + 1, 1);
  const double px = (double)grid.x * grid.y * PW_GH * PW_GW;
  crg_prof_scope ps(ctx, st, CRG_K_ELEMENTWISE, px * (20.0 + 12.0 * C), px * C * (4.0 * esz + 1.0));
  if (face_f32) hipLaunchKernelGGL(paste_warped_kernel<true>, grid, dim3(256), 0, st, s, m, (unsigned char*)image, img_sy, img_sx, H, W, tx0, ty0);
  else hipLaunchKernelGGL(paste_warped_kernel<false>, grid, dim3(256), 0, st, s, m, (unsigned char*)image, img_sy, img_sx, H, W, tx0, ty0);
  CRG_CHECK_LAUNCH(ctx, "paste_warped_u8");
  return 0;
}
