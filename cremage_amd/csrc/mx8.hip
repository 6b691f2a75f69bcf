// MX8: block-scaled e4m3 operands (one E8M0 scale per 32 elements along K) for the feed-forward GEMMs - the format paragraph is in
// include/crg_hip.h, the host restatement in cremage_amd/ops.py (quant_mx8_host).  Opt-in (FeedForward(precision="mx8")): no default
// path reaches this file.
//
// Operand layout of v_mfma_scale_f32_16x16x128_f8f6f4, measured with exact data (tools/probes/mx_scale_map.hip): lane l supplies row /
// column l & 15; with g = l >> 4, its registers 0..3 hold the 16 bytes k = 16 g .. 16 g + 15 and its registers 4..7 the 16 bytes
// k = 64 + 16 g .. 64 + 16 g + 15; byte 0 of its scale register (op_sel 0) scales the 32-element block k = 32 g .. 32 g + 31 of its row -
// i.e. the scale lanes follow the logical blocks while the data lanes interleave the two 64-byte halves.  C/D: col = l & 15,
// row = 4 (l >> 4) + r as for every 16x16 shape.
#include "crg_common.h"

typedef int mx_v8i __attribute__((ext_vector_type(8)));

// ---- the scale rule ---------------------------------------------------------------------------------------------------------------------
// E8M0 exponent of a block whose largest magnitude is a (finite, >= 0)
__device__ __forceinline__ int mx8_exp_of(float a) {
  const unsigned b = __float_as_uint(a);
  if (b == 0u) return 127;
  const int e = (int)(b >> 23) - 8 + ((b & 0x7fffffu) > 0x600000u ? 1 : 0);  // fp32 subnormals: field 0 -> negative -> clamped to 0
  return e < 0 ? 0 : (e > 254 ? 254 : e);
}
// 2^(127 - e) as a float: e <= 247 for every fp32 a, so the field stays >= 7
__device__ __forceinline__ float mx8_inv_scale(int e) { return __uint_as_float((unsigned)(254 - e) << 23); }
// four values already divided by the scale -> four codes, lowest byte first; a zero keeps no sign
__device__ __forceinline__ unsigned mx8_codes4(float a, float b, float c, float d) {
  const unsigned v = crg_pack4_e4m3(a, b, c, d);
  const unsigned nz = ((v & 0x7f7f7f7fu) + 0x7f7f7f7fu) & 0x80808080u;  // 0x80 in every byte whose magnitude bits are not all zero
  return v & (nz | 0x7f7f7f7fu);
}

// ---- quantiser: activations (geglu_f == 0) and Linear weights (geglu_f = F: the GEGLU row interleave of crg_pack_weight) ----------------
// One thread per 8 consecutive elements, four neighbouring lanes per 32-element block.
template <typename ST, bool VEC>
__global__ __launch_bounds__(256) void mx8_quant_kernel(const ST* __restrict__ src, long ld, unsigned char* __restrict__ q,
                                                        unsigned char* __restrict__ e, long rows, int K, int geglu_f) {
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;
  const int k8 = K >> 3;
  if (idx >= rows * k8) return;  // rows * k8 is a multiple of 4: a block's four lanes leave together
  const long o = idx / k8;
  const int c = (int)(idx - o * k8) * 8;
  long srow = o;
  if (geglu_f > 0) {  // packed row o: group o / 32, r = o % 32 -> source row 16 (o / 32) + r % 16 + (r / 16) F
    const long g = o >> 5;
    const int r = (int)(o & 31);
    srow = g * 16 + (r & 15) + (long)(r >> 4) * geglu_f;
  }
  const ST* p = src + srow * ld + c;
  float f[8];
  if constexpr (!VEC) {
#pragma unroll
    for (int i = 0; i < 8; ++i) f[i] = (float)p[i];
  } else if constexpr (sizeof(ST) == 4) {
    const f32x4 lo = *reinterpret_cast<const f32x4*>(p), hi = *reinterpret_cast<const f32x4*>(p + 4);
#pragma unroll
    for (int i = 0; i < 4; ++i) { f[i] = lo[i]; f[4 + i] = hi[i]; }
  } else {
    typedef ST st8 __attribute__((ext_vector_type(8)));
    const st8 v = *reinterpret_cast<const st8*>(p);
#pragma unroll
    for (int i = 0; i < 8; ++i) f[i] = (float)v[i];
  }
  float a = 0.f;
#pragma unroll
  for (int i = 0; i < 8; ++i) a = __builtin_fmaxf(a, __builtin_fabsf(f[i]));
  a = __builtin_fmaxf(a, __shfl_xor(a, 1));
  a = __builtin_fmaxf(a, __shfl_xor(a, 2));
  const int ex = mx8_exp_of(a);
  const float inv = mx8_inv_scale(ex);
  uint2 w;
  w.x = mx8_codes4(f[0] * inv, f[1] * inv, f[2] * inv, f[3] * inv);
  w.y = mx8_codes4(f[4] * inv, f[5] * inv, f[6] * inv, f[7] * inv);
  *reinterpret_cast<uint2*>(q + o * K + c) = w;
  if ((c & 31) == 0) e[o * (K >> 5) + (c >> 5)] = (unsigned char)ex;
}

template <typename ST>
static void mx8_quant_launch(hipStream_t st, const void* src, long ld, void* q, void* e, long rows, int K, int geglu_f) {
  const long threads = rows * (K / 8);
  const unsigned grid = (unsigned)((threads + 255) / 256);
  const bool vec = ((uintptr_t)src % 16 == 0) && ((ld * (long)sizeof(ST)) % 16 == 0);
  if (vec)
    hipLaunchKernelGGL((mx8_quant_kernel<ST, true>), dim3(grid), dim3(256), 0, st, (const ST*)src, ld, (unsigned char*)q, (unsigned char*)e, rows, K, geglu_f);
  else
    hipLaunchKernelGGL((mx8_quant_kernel<ST, false>), dim3(grid), dim3(256), 0, st, (const ST*)src, ld, (unsigned char*)q, (unsigned char*)e, rows, K, geglu_f);
}

extern "C" int crg_quant_mx8(crg_ctx* ctx, void* stream, const void* x, int64_t ldx, void* q, void* e, int64_t M, int K) {
  if (!ctx) return -22;
  CRG_REQUIRE(ctx, x && q && e && M > 0 && K > 0, "quant_mx8: bad arguments");
  CRG_REQUIRE(ctx, K % 32 == 0 && ldx >= K, "quant_mx8: K %% 32 == 0 and ldx >= K expected (K %d, ldx %lld)", K, (long long)ldx);
  CRG_REQUIRE(ctx, (uintptr_t)q % 8 == 0, "quant_mx8: q must be 8-byte aligned");
  CRG_REQUIRE(ctx, M * (K / 8) < (1LL << 38), "quant_mx8: %lld x %d is too large for one launch", (long long)M, K);
  hipStream_t st = (hipStream_t)stream;
  crg_prof_scope ps(ctx, st, CRG_K_ELEMENTWISE, 4.0 * M * K, (double)M * K * (2.0 + 1.0 + 1.0 / 32));
  mx8_quant_launch<bf16>(st, x, ldx, q, e, M, K, 0);
  CRG_CHECK_LAUNCH(ctx, "quant_mx8");
  return 0;
}

extern "C" int crg_pack_weight_mx8(crg_ctx* ctx, void* stream, const void* src, int src_dtype, int kind, int n_out, int n_in, void* dst_q,
                                   void* dst_e) {
  if (!ctx) return -22;
  CRG_REQUIRE(ctx, src && dst_q && dst_e && n_out > 0 && n_in > 0, "pack_weight_mx8: bad arguments");
  CRG_REQUIRE(ctx, kind == CRG_PACK_LINEAR || kind == CRG_PACK_GEGLU, "pack_weight_mx8: kind %d unsupported", kind);
  CRG_REQUIRE(ctx, n_in % 32 == 0, "pack_weight_mx8: n_in %% 32 == 0 expected, got %d", n_in);
  if (kind == CRG_PACK_GEGLU) CRG_REQUIRE(ctx, n_out % 32 == 0, "pack_weight_mx8: GEGLU needs n_out %% 32 == 0, got %d", n_out);
  CRG_REQUIRE(ctx, (uintptr_t)dst_q % 8 == 0, "pack_weight_mx8: dst_q must be 8-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  const int f = kind == CRG_PACK_GEGLU ? n_out / 2 : 0;
  if (src_dtype == CRG_F32) mx8_quant_launch<float>(st, src, n_in, dst_q, dst_e, n_out, n_in, f);
  else if (src_dtype == CRG_BF16) mx8_quant_launch<bf16>(st, src, n_in, dst_q, dst_e, n_out, n_in, f);
#ifndef CRG_F16_BUILD
  else if (src_dtype == CRG_F16) mx8_quant_launch<_Float16>(st, src, n_in, dst_q, dst_e, n_out, n_in, f);
#endif
  else return crg_fail(ctx, -22, "pack_weight_mx8: unsupported source dtype %d", src_dtype);
  CRG_CHECK_LAUNCH(ctx, "pack_weight_mx8");
  return 0;
}

// ---- GEMM -------------------------------------------------------------------------------------------------------------------------------
// The matrix instruction's A operand is W and its B operand the activations, so a lane's four accumulators are four CONSECUTIVE output
// columns of one row: 8-byte (half) / 16-byte (fp32) / 4-byte (codes) stores, and the 32-column absmax of the MX8 output is two tiles in
// the lane plus two cross-lane steps.  Operands go from global memory (L1 / L2) straight to registers, 16 bytes per load, the next k-step
// in flight under the current one's MFMAs (two fragment sets in turn), every step multiplied in four passes (below); a wave owns 64 rows x 64 packed columns (16 accumulator tiles), a block 2 x 2 waves.
#define MX8_TM 4  // 16-row tiles of the activations per wave (2 and 3 with two waves per SIMD measured no faster: DESIGN 6 f13)
#define MX8_TN 4  // 16-row tiles of W per wave (four: value | gate | value | gate = one 32-column block of a GEGLU MX8 output)
#define MX8_BM (2 * 16 * MX8_TM)
#define MX8_BN (2 * 16 * MX8_TN)

struct mx8_frag {
  mx_v8i v;
  int s;
};

// One operand fragment of the k-step at k0.  Branch-free and with nothing computed FROM the loaded bytes, so that the loads of the next
// step stay in flight under this step's instructions (the compiler waits for a load where its first reader is scheduled): K % 128 == 64
// leaves the last step without its second half, which is then read from the context's page of zeros; a block past the end takes the
// row's last scale, which multiplies those zeros.
__device__ __forceinline__ mx8_frag mx8_load(const unsigned char* __restrict__ qrow, const unsigned char* __restrict__ erow,
                                             const unsigned char* __restrict__ zeros, int k0, int K, int g) {
  mx8_frag f;
  const int4 lo = *reinterpret_cast<const int4*>(qrow + k0 + 16 * g);
  const int4 hi = *reinterpret_cast<const int4*>((k0 + 64 < K ? qrow + k0 + 64 : zeros) + 16 * g);
  f.v[0] = lo.x; f.v[1] = lo.y; f.v[2] = lo.z; f.v[3] = lo.w;
  f.v[4] = hi.x; f.v[5] = hi.y; f.v[6] = hi.z; f.v[7] = hi.w;
  f.s = (int)erow[min((k0 >> 5) + g, (K >> 5) - 1)];
  return f;
}

// The codes of a fragment as two fragments: magnitudes >= 16.0 (field 0x58) and the rest; the other bytes are +0.
__device__ __forceinline__ void mx8_split(const mx_v8i& v, mx_v8i& big, mx_v8i& small) {
#pragma unroll
  for (int q = 0; q < 8; ++q) {
    const unsigned x = (unsigned)v[q];
    const unsigned ge = ((x & 0x7f7f7f7fu) + 0x28282828u) & 0x80808080u;  // 0x80 in every byte whose magnitude field is >= 0x58
    const unsigned m = (ge >> 7) * 0xffu;
    big[q] = (int)(x & m);
    small[q] = (int)(x & ~m);
  }
}

template <bool GEGLU, int YK>
__global__ __launch_bounds__(256) void mx8_gemm_kernel(const crg_mx8gemm_args p, const unsigned char* __restrict__ zeros) {
  const int l = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int c = l & 15, g = l >> 4;
  const int m0 = blockIdx.y * MX8_BM + (wave >> 1) * (16 * MX8_TM);
  const int n0 = blockIdx.x * MX8_BN + (wave & 1) * (16 * MX8_TN);
  if (m0 >= p.M || n0 >= p.N) return;  // wave-uniform; no barrier follows
  const int K = p.K, KB = K >> 5;
  const unsigned char* aq[MX8_TM];
  const unsigned char* ae[MX8_TM];
  const unsigned char* wq[MX8_TN];
  const unsigned char* we[MX8_TN];
#pragma unroll
  for (int t = 0; t < MX8_TM; ++t) {  // rows past the end read the last row; their results are never stored
    const long m = min(m0 + 16 * t + c, p.M - 1);
    aq[t] = (const unsigned char*)p.a_q + m * p.lda;
    ae[t] = (const unsigned char*)p.a_e + m * p.lde;
  }
#pragma unroll
  for (int t = 0; t < MX8_TN; ++t) {
    const long n = min(n0 + 16 * t + c, p.N - 1);
    wq[t] = (const unsigned char*)p.w_q + n * K;
    we[t] = (const unsigned char*)p.w_e + n * KB;
  }
  f32x4 acc[MX8_TM][MX8_TN];
#pragma unroll
  for (int i = 0; i < MX8_TM; ++i)
#pragma unroll
    for (int j = 0; j < MX8_TN; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  // two fragment sets in turn: set 1 loads while set 0 multiplies and the other way round - no copies, so each multiply waits only for
  // its own set.  Past the last step the prefetch re-reads an earlier step (in bounds, never used).
#define MX8_LOAD(FA, FW, K0)                                                                          \
  _Pragma("unroll") for (int t = 0; t < MX8_TM; ++t) FA[t] = mx8_load(aq[t], ae[t], zeros, K0, K, g); \
  _Pragma("unroll") for (int t = 0; t < MX8_TN; ++t) FW[t] = mx8_load(wq[t], we[t], zeros, K0, K, g);
  // Every k-step is multiplied in FOUR passes, large x large, large x small, small x large, small x small codes (mx8_split): the
  // instruction keeps only so many bits below the largest product of a 32-element block, and one pass loses the small products of a
  // block that holds an outlier.  Matrix work x 4 in a loop that the operand path bounds; the sums are those of one pass, more exactly.
#define MX8_ONE(I, J, W, A, FA, FW) acc[I][J] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(W, A, acc[I][J], 0, 0, 0, FW[J].s, 0, FA[I].s);
#define MX8_MMA(FA, FW)                                                                   \
  {                                                                                       \
    mx_v8i wb[MX8_TN], ws[MX8_TN];                                                        \
    _Pragma("unroll") for (int j = 0; j < MX8_TN; ++j) mx8_split(FW[j].v, wb[j], ws[j]);  \
    _Pragma("unroll") for (int i = 0; i < MX8_TM; ++i) {                                  \
      mx_v8i ab, as;                                                                      \
      mx8_split(FA[i].v, ab, as);                                                         \
      _Pragma("unroll") for (int j = 0; j < MX8_TN; ++j) { MX8_ONE(i, j, wb[j], ab, FA, FW) } \
      _Pragma("unroll") for (int j = 0; j < MX8_TN; ++j) { MX8_ONE(i, j, wb[j], as, FA, FW) } \
      _Pragma("unroll") for (int j = 0; j < MX8_TN; ++j) { MX8_ONE(i, j, ws[j], ab, FA, FW) } \
      _Pragma("unroll") for (int j = 0; j < MX8_TN; ++j) { MX8_ONE(i, j, ws[j], as, FA, FW) } \
    }                                                                                     \
  }
  mx8_frag fa0[MX8_TM], fw0[MX8_TN], fa1[MX8_TM], fw1[MX8_TN];
  MX8_LOAD(fa0, fw0, 0)
  const int Kr = (K + 127) & ~127;
  int k0 = 0;
  for (; k0 + 256 <= Kr; k0 += 256) {  // two steps per trip, one exit at the bottom: a single straight-line body
    MX8_LOAD(fa1, fw1, k0 + 128)
    MX8_MMA(fa0, fw0)
    MX8_LOAD(fa0, fw0, (k0 + 256 < K ? k0 + 256 : k0))
    MX8_MMA(fa1, fw1)
  }
  if (k0 < K) {  // an odd number of steps: the last one is in set 0
    MX8_MMA(fa0, fw0)
  }
#undef MX8_LOAD
#undef MX8_ONE
#undef MX8_MMA
  // ---- epilogue: acc[i][j][r] = row m0 + 16 i + c, packed column n0 + 16 j + 4 g + r ----
  constexpr int TO = GEGLU ? MX8_TN / 2 : MX8_TN;  // output tiles of 16 columns
  const int oc0 = (GEGLU ? n0 / 2 : n0) + 4 * g;   // this lane's first output column in tile 0
#pragma unroll
  for (int i = 0; i < MX8_TM; ++i) {
    const int m = m0 + 16 * i + c;
    const bool mok = m < p.M;
    f32x4 v[TO];
#pragma unroll
    for (int j = 0; j < TO; ++j) {
      if constexpr (GEGLU) {
        const int pn = n0 + 32 * j + 4 * g;  // packed column of the value tile; the gate tile sits 16 further
        f32x4 bv = {0.f, 0.f, 0.f, 0.f}, bg = bv;
        if (p.bias && pn < p.N) {
          bv = *reinterpret_cast<const f32x4*>(p.bias + pn);
          bg = *reinterpret_cast<const f32x4*>(p.bias + pn + 16);
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) v[j][r] = (acc[i][2 * j][r] + bv[r]) * crg_gelu_erf_f(acc[i][2 * j + 1][r] + bg[r]);
      } else {
        const int pn = n0 + 16 * j + 4 * g;
        v[j] = acc[i][j];
        if (pn < p.N) {
          if (p.bias) {
            const f32x4 b = *reinterpret_cast<const f32x4*>(p.bias + pn);
#pragma unroll
            for (int r = 0; r < 4; ++r) v[j][r] += b[r];
          }
          if (p.residual && mok) {
            const bf16x4 rr = *reinterpret_cast<const bf16x4*>((const bf16*)p.residual + (long)m * p.ldr + pn);
#pragma unroll
            for (int r = 0; r < 4; ++r) v[j][r] += (float)rr[r];
          }
        }
      }
    }
    const int NO = GEGLU ? p.N / 2 : p.N;
    if constexpr (YK == CRG_MX8_OUT_MX8) {
#pragma unroll
      for (int b = 0; b < TO / 2; ++b) {  // blocks of 32 output columns: tiles 2 b and 2 b + 1, all four lane groups
        float a = 0.f;
#pragma unroll
        for (int r = 0; r < 4; ++r) a = __builtin_fmaxf(a, __builtin_fmaxf(__builtin_fabsf(v[2 * b][r]), __builtin_fabsf(v[2 * b + 1][r])));
        a = __builtin_fmaxf(a, __shfl_xor(a, 16));
        a = __builtin_fmaxf(a, __shfl_xor(a, 32));
        const int ex = mx8_exp_of(a);
        const float inv = mx8_inv_scale(ex);
        const int oc = oc0 + 32 * b;
        if (mok && oc < NO) {  // NO % 64 == 0: a block is inside or outside as a whole
          unsigned char* yq = (unsigned char*)p.y + (long)m * p.ldy;
#pragma unroll
          for (int h = 0; h < 2; ++h)
            *reinterpret_cast<unsigned*>(yq + oc + 16 * h) =
                mx8_codes4(v[2 * b + h][0] * inv, v[2 * b + h][1] * inv, v[2 * b + h][2] * inv, v[2 * b + h][3] * inv);
          if (g == 0) ((unsigned char*)p.y_e)[(long)m * p.ldye + (oc >> 5)] = (unsigned char)ex;
        }
      }
    } else {
#pragma unroll
      for (int j = 0; j < TO; ++j) {
        const int oc = oc0 + 16 * j;
        if (!mok || oc >= NO) continue;
        if constexpr (YK == CRG_MX8_OUT_F32) {
          *reinterpret_cast<f32x4*>((float*)p.y + (long)m * p.ldy + oc) = v[j];
        } else {
          bf16x4 o;
#pragma unroll
          for (int r = 0; r < 4; ++r) o[r] = (bf16)v[j][r];
          *reinterpret_cast<bf16x4*>((bf16*)p.y + (long)m * p.ldy + oc) = o;
        }
      }
    }
  }
}

extern "C" int crg_gemm_mx8(crg_ctx* ctx, void* stream, const crg_mx8gemm_args* a) {
  if (!ctx) return -22;
  CRG_REQUIRE(ctx, a && a->a_q && a->a_e && a->w_q && a->w_e && a->y, "gemm_mx8: bad arguments");
  CRG_REQUIRE(ctx, a->M > 0 && a->N > 0 && a->K > 0, "gemm_mx8: empty problem (%d x %d x %d)", a->M, a->N, a->K);
  CRG_REQUIRE(ctx, a->K % 64 == 0, "gemm_mx8: K %% 64 == 0 expected, got %d", a->K);
  CRG_REQUIRE(ctx, a->N % 32 == 0, "gemm_mx8: N %% 32 == 0 expected, got %d", a->N);
  CRG_REQUIRE(ctx, a->epilogue == CRG_EPI_NONE || a->epilogue == CRG_EPI_GEGLU, "gemm_mx8: epilogue %d unsupported", a->epilogue);
  CRG_REQUIRE(ctx, a->y_kind >= CRG_MX8_OUT_HALF && a->y_kind <= CRG_MX8_OUT_MX8, "gemm_mx8: y_kind %d unsupported", a->y_kind);
  const bool geglu = a->epilogue == CRG_EPI_GEGLU;
  const int n_out = geglu ? a->N / 2 : a->N;
  CRG_REQUIRE(ctx, !(geglu && a->residual), "gemm_mx8: the GEGLU epilogue takes no residual");
  CRG_REQUIRE(ctx, a->lda >= a->K && a->lda % 16 == 0 && (uintptr_t)a->a_q % 16 == 0 && (uintptr_t)a->w_q % 16 == 0,
              "gemm_mx8: code planes need 16-byte aligned rows (lda %lld)", (long long)a->lda);
  CRG_REQUIRE(ctx, a->lde >= a->K / 32, "gemm_mx8: lde %lld below K / 32", (long long)a->lde);
  CRG_REQUIRE(ctx, a->ldy >= n_out && a->ldy % 4 == 0 && (uintptr_t)a->y % 16 == 0, "gemm_mx8: y needs ldy %% 4 == 0 and a 16-byte aligned base");
  CRG_REQUIRE(ctx, !a->bias || (uintptr_t)a->bias % 16 == 0, "gemm_mx8: bias must be 16-byte aligned");
  if (a->residual) CRG_REQUIRE(ctx, a->ldr >= n_out && a->ldr % 4 == 0 && (uintptr_t)a->residual % 8 == 0, "gemm_mx8: residual needs ldr %% 4 == 0 and an 8-byte aligned base");
  if (a->y_kind == CRG_MX8_OUT_MX8) {
    CRG_REQUIRE(ctx, n_out % 64 == 0, "gemm_mx8: an MX8 output needs a width that is a multiple of 64, got %d", n_out);
    CRG_REQUIRE(ctx, a->y_e && a->ldye >= n_out / 32, "gemm_mx8: an MX8 output needs y_e with ldye >= width / 32");
  }
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((a->N + MX8_BN - 1) / MX8_BN, (a->M + MX8_BM - 1) / MX8_BM);
  const double ysz = a->y_kind == CRG_MX8_OUT_F32 ? 4.0 : a->y_kind == CRG_MX8_OUT_HALF ? 2.0 : 1.0 + 1.0 / 32;
  crg_prof_scope ps(ctx, st, CRG_K_GEMM_W1, 2.0 * a->M * a->N * a->K,
                    ((double)a->M + a->N) * a->K * (1.0 + 1.0 / 32) + (double)a->M * n_out * (ysz + (a->residual ? 2.0 : 0.0)));
#define MX8_LAUNCH(G, Y) hipLaunchKernelGGL((mx8_gemm_kernel<G, Y>), grid, dim3(256), 0, st, *a, (const unsigned char*)ctx->zero_page)
  if (geglu) {
    if (a->y_kind == CRG_MX8_OUT_HALF) MX8_LAUNCH(true, CRG_MX8_OUT_HALF);
    else if (a->y_kind == CRG_MX8_OUT_F32) MX8_LAUNCH(true, CRG_MX8_OUT_F32);
    else MX8_LAUNCH(true, CRG_MX8_OUT_MX8);
  } else {
    if (a->y_kind == CRG_MX8_OUT_HALF) MX8_LAUNCH(false, CRG_MX8_OUT_HALF);
    else if (a->y_kind == CRG_MX8_OUT_F32) MX8_LAUNCH(false, CRG_MX8_OUT_F32);
    else MX8_LAUNCH(false, CRG_MX8_OUT_MX8);
  }
#undef MX8_LAUNCH
  CRG_CHECK_LAUNCH(ctx, "gemm_mx8");
  return 0;
}
