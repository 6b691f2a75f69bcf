// Dev probe (standalone): which lane's scale register v_mfma_scale_f32_16x16x128_f8f6f4 applies to which operand bytes, found with exact
// data.  mx_layout.hip confirmed the data layout only up to a k-permutation shared by A and B (uniform and per-row scales came out right,
// per-k-block scales did not), so the scale map is measured here instead of assumed:
//   one operand holds 1.0 (e4m3 0x38) in ONE register q of ONE 16-lane group g and zeros elsewhere, the other holds 1.0 everywhere; every
//   scale is 2^0 except lane L's, which is 2^1.  Each output the marked bytes reach is 4 when lane L's scale does not apply to them and 8
//   when it does.  The table (g, q) -> set of L says which lane scales which bytes; the printed summary names every L that moved a result.
// mode 0: A varied (rows), mode 1: B varied (columns).  Last: the three upper bytes of the scale register are ignored under op_sel 0.
// Build: hipcc --offload-arch=gfx950 -O3 mx_scale_map.hip -o mx_scale_map
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <string.h>
typedef int v8i __attribute__((ext_vector_type(8)));
typedef float v4f __attribute__((ext_vector_type(4)));

// out[((g * 8 + q) * 64 + L) * 16 + i]: the result of row (mode 0) / column (mode 1) i
__global__ void scale_map(float* out, int mode) {
  const int l = threadIdx.x;
  for (int g = 0; g < 4; ++g)
    for (int q = 0; q < 8; ++q)
      for (int L = 0; L < 64; ++L) {
        v8i one, var;
        for (int r = 0; r < 8; ++r) {
          one[r] = 0x38383838;
          var[r] = ((l >> 4) == g && r == q) ? 0x38383838 : 0;
        }
        const int sv = l == L ? 128 : 127, s1 = 127;
        v4f acc = {0.f, 0.f, 0.f, 0.f};
        if (mode == 0) acc = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(var, one, acc, 0, 0, 0, sv, 0, s1);
        else acc = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(one, var, acc, 0, 0, 0, s1, 0, sv);
        float* o = out + ((size_t)((g * 8 + q) * 64 + L)) * 16;
        if (mode == 0) {  // C/D: col = l & 15, row = 4 (l >> 4) + r; column 0 holds every row
          if ((l & 15) == 0)
            for (int r = 0; r < 4; ++r) o[4 * (l >> 4) + r] = acc[r];
        } else {
          if ((l >> 4) == 0) o[l & 15] = acc[0];  // row 0 holds every column
        }
      }
}

__global__ void upper_bytes(float* out) {
  v8i one;
  for (int r = 0; r < 8; ++r) one[r] = 0x38383838;
  const int s = 127 | (130 << 8) | (131 << 16) | (132 << 24);
  v4f acc = {0.f, 0.f, 0.f, 0.f};
  acc = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(one, one, acc, 0, 0, 0, s, 0, s);
  out[threadIdx.x] = acc[0];
}

int main() {
  const size_t n = 4 * 8 * 64 * 16;
  float* d;
  if (hipMalloc(&d, n * sizeof(float)) != hipSuccess) { printf("no device\n"); return 1; }
  static float h[4 * 8 * 64 * 16];
  for (int mode = 0; mode < 2; ++mode) {
    hipMemset(d, 0, n * sizeof(float));
    hipLaunchKernelGGL(scale_map, dim3(1), dim3(64), 0, 0, d, mode);
    if (hipMemcpy(h, d, n * sizeof(float), hipMemcpyDeviceToHost) != hipSuccess) { printf("copy failed\n"); return 1; }
    printf("mode %d (%s varied): bytes of lane group g, register q <- the lanes L whose scale moved a result [L:index, ...]\n", mode, mode ? "B" : "A");
    for (int g = 0; g < 4; ++g)
      for (int q = 0; q < 8; ++q) {
        printf("  g %d q %d:", g, q);
        int odd = 0;
        for (int L = 0; L < 64; ++L)
          for (int i = 0; i < 16; ++i) {
            const float v = h[((size_t)((g * 8 + q) * 64 + L)) * 16 + i];
            if (v == 8.f) printf(" %d:%d", L, i);
            else if (v != 4.f) ++odd;
          }
        printf(odd ? "   (%d results neither 4 nor 8)\n" : "\n", odd);
      }
  }
  hipLaunchKernelGGL(upper_bytes, dim3(1), dim3(64), 0, 0, d);
  hipMemcpy(h, d, 64 * sizeof(float), hipMemcpyDeviceToHost);
  printf("upper scale bytes set, op_sel 0: D[0][0] = %g (128 = ignored)\n", h[0]);
  hipFree(d);
  return 0;
}
