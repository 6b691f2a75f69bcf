// Flash attention for the fp32 class ("x3"): O = softmax(Q K^T * scale) V on fp32 tensors, every product taken as three half-type
// MFMA passes over hi / lo planes, in ONE launch and with no score buffer (see include/crg_hip.h, crg_attention_x3).
//
// Structure.  A block is four waves of 16 query rows each (64 rows) of one (batch, head); it walks the keys in tiles of 32.
//   * Q: each wave keeps the hi and lo planes of its 16 rows in registers for the whole kernel (split once, from fp32).
//   * K and V^T tiles: read as fp32, split into hi / lo planes while they are staged into LDS.  Keys >= Nk and channels >= Dh are
//     written as zeros BY SELECTION - their memory is never read - so nothing behind a tail can reach a product.
//   * Both products run transposed, so that a query stays on one lane column from the first MFMA to the store:
//       S^T = K Q^T   A = K tile [16 keys][32 d], B = Q^T: result col = lane & 15 = query, row = 4 (lane >> 4) + r = key
//       O^T = V^T P^T A = V^T tile [16 d][32 keys], B = P^T: result col = query, row = channel
//     The S^T registers of a lane ARE its fragment of P^T (keys 4g + r of the two 16-key halves): no LDS round trip, no lane
//     movement.  The k index of that MFMA is therefore a permutation of the tile's keys (slot 8g + 4h + r = key 16h + 4g + r);
//     the V^T tile is staged in the same slot order, which also makes a lane's eight keys one 16-byte LDS read.
//   * Online softmax in fp32: running max and row sum per query (identical on the four lanes of a column after two xor shuffles),
//     exp2 of (logit - max) * (scale log2 e), O rescaled by exp2(old max - new max) before each tile's products.  The max of the
//     first tile replaces -inf, whose factor is exp2(-inf) = 0 on a zero accumulator: no NaN.  Masked keys get P = 0 by selection.
//   * Two barriers per key tile.  The loads of a tile lie under the other product: V^T of tile t is fetched and staged in pieces
//     between the MFMA groups of S^T(t), K of tile t + 1 between those of the PV product of tile t, a few registers at a time.
// Deterministic: no atomics, keys are never split across blocks, every sum has a fixed order.
#include "crg_common.h"

namespace {
constexpr int AX_ROWS = 64;   // query rows per block (4 waves x 16)
constexpr int AX_KEYS = 32;   // keys per tile
constexpr int AX_VLD = 40;    // key slots per V^T row in LDS (32 + 8 pad: 80-byte rows, 16-byte aligned)

template <int DP>
struct ax_cfg {
  static constexpr int KLD = DP + 8;              // elements per K row in LDS (16 bytes of pad)
  static constexpr int K_PLANE = AX_KEYS * KLD;   // elements
  static constexpr int V_PLANE = DP * AX_VLD;
  static constexpr size_t LDS = (size_t)(2 * K_PLANE + 2 * V_PLANE) * sizeof(bf16);
  static_assert(DP % 32 == 0 && DP <= 512, "padded head dim: whole 32-channel MFMA steps");
  static_assert(LDS <= 160 * 1024, "LDS budget of one block");
};

__device__ __forceinline__ void ax_split4(const f32x4 f, bf16x4& h, bf16x4& l) {
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    h[e] = (bf16)f[e];
    l[e] = (bf16)(f[e] - (float)h[e]);
  }
}

// DP: Dh rounded up to an instantiated multiple of 32.  sl2 = scale * log2(e).  vec_v: V^T rows may be read as float4.
template <int DP>
__global__ __launch_bounds__(256) void attn_x3_kernel(const crg_attn_x3_args p, const float sl2, const int vec_v) {
  using cfg = ax_cfg<DP>;
  constexpr int KLD = cfg::KLD, KS = DP / 32, DT = DP / 16;
  extern __shared__ __attribute__((aligned(16))) unsigned char ax_smem[];
  bf16* const kh = reinterpret_cast<bf16*>(ax_smem);
  bf16* const kl = kh + cfg::K_PLANE;
  bf16* const vh = kl + cfg::K_PLANE;
  bf16* const vl = vh + cfg::V_PLANE;

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, c = lane & 15, g = lane >> 4;
  const int head = blockIdx.y, b = blockIdx.z;
  const int Dh = p.Dh, Nk = p.Nk;
  const int q_row = blockIdx.x * AX_ROWS + wave * 16 + c;
  const bool q_ok = q_row < p.Nq;
  const float* const K = p.k + (long)b * Nk * p.ldk + (long)head * Dh;
  const float* const VT = p.vt + ((long)b * p.H + head) * Dh * p.ldvt;

  // Q^T fragments: element j of step s is Q[q_row][32 s + 8 g + j]
  bf16x8 qh[KS], ql[KS];
  {
    const float* const qp = p.q + ((long)b * p.Nq + q_row) * p.ldq + (long)head * Dh;
#pragma unroll
    for (int s = 0; s < KS; ++s) {
      const int d = 32 * s + 8 * g;
      f32x4 f0 = {0.f, 0.f, 0.f, 0.f}, f1 = f0;
      if (q_ok && d < Dh) {
        f0 = *reinterpret_cast<const f32x4*>(qp + d);
        f1 = *reinterpret_cast<const f32x4*>(qp + d + 4);
      }
      bf16x4 h0, l0, h1, l1;
      ax_split4(f0, h0, l0);
      ax_split4(f1, h1, l1);
      qh[s] = __builtin_shufflevector(h0, h1, 0, 1, 2, 3, 4, 5, 6, 7);
      ql[s] = __builtin_shufflevector(l0, l1, 0, 1, 2, 3, 4, 5, 6, 7);
    }
  }

  f32x4 acc[DT];
#pragma unroll
  for (int i = 0; i < DT; ++i) acc[i] = f32x4{0.f, 0.f, 0.f, 0.f};
  float m = -__builtin_inff(), l = 0.f;

  // Staging, one float4 piece at a time: the load is issued before a group of MFMAs and the split + LDS write follows it, so the
  // flight of a tile's loads lies under the other product of the loop (see the tile loop).  A thread keeps ONE column position
  // per operand and steps through rows, so a piece's address is the tile's base pointer plus a wave-uniform offset; the base is
  // rebuilt per tile behind an empty asm, or the compiler keeps every piece's 64-bit address in registers across the loop
  // (32 pointers: spills at d_head 512).
  // K: [32 keys][DP]; TPR threads per row (the power of two >= DP / 4), 256 / TPR rows per piece, NPK pieces.
  constexpr int TPR = DP <= 64 ? 16 : DP <= 128 ? 32 : DP <= 256 ? 64 : 128, RPP = 256 / TPR, NPK = AX_KEYS / RPP;
  const int k_r0 = tid / TPR, k_d = (tid % TPR) * 4;
  const bool k_dok = k_d < Dh;  // false as well on the idle threads of a row (DP = 96, 160: k_d >= DP), which store nothing either
  auto k_base = [&](const int kbase) -> const float* {
    const float* ptr = K + (long)(kbase + k_r0) * p.ldk + k_d;
    asm volatile("" : "+v"(ptr));
    return ptr;
  };
  auto k_load = [&](const int i, const float* const base, const int kbase) -> f32x4 {
    f32x4 f = {0.f, 0.f, 0.f, 0.f};
    if (k_dok && kbase + k_r0 + RPP * i < Nk) f = *reinterpret_cast<const f32x4*>(base + (long)(RPP * i) * p.ldk);
    return f;
  };
  auto k_store = [&](const int i, const f32x4 f) {
    if (TPR * 4 != DP && k_d >= DP) return;
    bf16x4 h, lo;
    ax_split4(f, h, lo);
    *reinterpret_cast<bf16x4*>(kh + (k_r0 + RPP * i) * KLD + k_d) = h;
    *reinterpret_cast<bf16x4*>(kl + (k_r0 + RPP * i) * KLD + k_d) = lo;
  };
  // V^T: [DP channels][32 keys] in pieces of four keys; keys 16 h + 4 g .. + 3 land in slots 8 g + 4 h .. + 3.  32 channels per piece.
  const int v_d0 = tid >> 3, v_piece = tid & 7;
  auto v_base = [&](const int kbase) -> const float* {
    const float* ptr = VT + (long)v_d0 * p.ldvt + kbase + 4 * v_piece;
    asm volatile("" : "+v"(ptr));
    return ptr;
  };
  auto v_load = [&](const int i, const float* const base, const int kbase) -> f32x4 {
    const int key = kbase + 4 * v_piece;
    f32x4 f = {0.f, 0.f, 0.f, 0.f};
    if (v_d0 + 32 * i < Dh && key < Nk) {
      const float* const src = base + (long)(32 * i) * p.ldvt;
      if (vec_v && key + 3 < Nk) {
        f = *reinterpret_cast<const f32x4*>(src);
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
          if (key + e < Nk) f[e] = src[e];
      }
    }
    return f;
  };
  auto v_store = [&](const int i, const f32x4 f) {
    bf16x4 h, lo;
    ax_split4(f, h, lo);
    const int slot = 8 * (v_piece & 3) + 4 * (v_piece >> 2);
    *reinterpret_cast<bf16x4*>(vh + (v_d0 + 32 * i) * AX_VLD + slot) = h;
    *reinterpret_cast<bf16x4*>(vl + (v_d0 + 32 * i) * AX_VLD + slot) = lo;
  };
  // pieces per group of MFMAs; groups of the S^T product (V^T pieces: KS) and of the PV product (K pieces: NPK), PV tiles per group
  constexpr int CH = 4, NCH = (KS + CH - 1) / CH, NCHK = (NPK + CH - 1) / CH, TPC = (DT + NCHK - 1) / NCHK;

  {
    const float* const kb = k_base(0);
#pragma unroll 4
    for (int i = 0; i < NPK; ++i) k_store(i, k_load(i, kb, 0));  // K of the first tile
  }

  const int n_tiles = (Nk + AX_KEYS - 1) / AX_KEYS;
  for (int t = 0; t < n_tiles; ++t) {
    const int k0 = t * AX_KEYS;
    __syncthreads();  // K of this tile is staged; every wave is done with the previous tile's V^T

    // ---- S^T = K Q^T for the tile's two 16-key halves: Qh Kh + Qh Kl + Ql Kh; this tile's V^T is staged underneath
    f32x4 s0 = {0.f, 0.f, 0.f, 0.f}, s1 = s0;
    const float* const vb = v_base(k0);
#pragma unroll
    for (int ch = 0; ch < NCH; ++ch) {
      f32x4 buf[CH];
#pragma unroll
      for (int j = 0; j < CH; ++j)
        if (ch * CH + j < KS) buf[j] = v_load(ch * CH + j, vb, k0);
#pragma unroll
      for (int j = 0; j < CH; ++j) {
        const int s = ch * CH + j;
        if (s < KS) {
          const int off = c * KLD + 32 * s + 8 * g;
          const bf16x8 a0h = *reinterpret_cast<const bf16x8*>(kh + off);
          const bf16x8 a0l = *reinterpret_cast<const bf16x8*>(kl + off);
          const bf16x8 a1h = *reinterpret_cast<const bf16x8*>(kh + off + 16 * KLD);
          const bf16x8 a1l = *reinterpret_cast<const bf16x8*>(kl + off + 16 * KLD);
          s0 = CRG_MFMA_16x16x32(a0l, qh[s], s0);
          s0 = CRG_MFMA_16x16x32(a0h, ql[s], s0);
          s0 = CRG_MFMA_16x16x32(a0h, qh[s], s0);
          s1 = CRG_MFMA_16x16x32(a1l, qh[s], s1);
          s1 = CRG_MFMA_16x16x32(a1h, ql[s], s1);
          s1 = CRG_MFMA_16x16x32(a1h, qh[s], s1);
        }
      }
#pragma unroll
      for (int j = 0; j < CH; ++j)
        if (ch * CH + j < KS) v_store(ch * CH + j, buf[j]);
      __builtin_amdgcn_sched_barrier(0);  // keep the next group's loads behind this group (registers)
    }

    // ---- online softmax of this lane's eight keys of query column c
    float tv[8];
    bool ok[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      ok[j] = k0 + 16 * (j >> 2) + 4 * g + (j & 3) < Nk;
      const float sv = j < 4 ? s0[j] : s1[j - 4];
      tv[j] = ok[j] ? sv * sl2 : -__builtin_inff();
    }
    float mt = tv[0];
#pragma unroll
    for (int j = 1; j < 8; ++j) mt = __builtin_fmaxf(mt, tv[j]);
    mt = __builtin_fmaxf(mt, __shfl_xor(mt, 16));
    mt = __builtin_fmaxf(mt, __shfl_xor(mt, 32));
    const float m_new = __builtin_fmaxf(m, mt);
    const float m_ref = m_new == -__builtin_inff() ? 0.f : m_new;  // a row of -inf logits: exp2(-inf - 0) = 0, not exp2(NaN)
    const float alpha = __builtin_amdgcn_exp2f(m - m_ref);
    m = m_new;
    bf16x8 ph, pl;
    float sum = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      const float pv = ok[j] ? __builtin_amdgcn_exp2f(tv[j] - m_ref) : 0.f;
      sum += pv;
      ph[j] = (bf16)pv;
      pl[j] = (bf16)(pv - (float)ph[j]);
    }
    l = l * alpha + sum;  // this lane's part of the row sum: the four lanes of a column share alpha, the parts are added at the end

    __syncthreads();  // V^T of this tile is staged; every wave is done with this tile's K

    // ---- O^T = O^T * alpha + V^T P^T: Ph Vh + Ph Vl + Pl Vh; the next tile's K is staged underneath (keys >= Nk: zeros, no reads)
    const float* const kb = k_base(k0 + AX_KEYS);
#pragma unroll
    for (int ch = 0; ch < NCHK; ++ch) {
      f32x4 buf[CH];
#pragma unroll
      for (int j = 0; j < CH; ++j)
        if (ch * CH + j < NPK) buf[j] = k_load(ch * CH + j, kb, k0 + AX_KEYS);
#pragma unroll
      for (int j = 0; j < TPC; ++j) {
        const int i = ch * TPC + j;
        if (i < DT) {
          const int off = (16 * i + c) * AX_VLD + 8 * g;
          const bf16x8 ah = *reinterpret_cast<const bf16x8*>(vh + off);
          const bf16x8 al = *reinterpret_cast<const bf16x8*>(vl + off);
#pragma unroll
          for (int r = 0; r < 4; ++r) acc[i][r] *= alpha;
          acc[i] = CRG_MFMA_16x16x32(al, ph, acc[i]);
          acc[i] = CRG_MFMA_16x16x32(ah, pl, acc[i]);
          acc[i] = CRG_MFMA_16x16x32(ah, ph, acc[i]);
        }
      }
#pragma unroll
      for (int j = 0; j < CH; ++j)
        if (ch * CH + j < NPK) k_store(ch * CH + j, buf[j]);
      __builtin_amdgcn_sched_barrier(0);
    }
  }

  l += __shfl_xor(l, 16);
  l += __shfl_xor(l, 32);
  if (!q_ok) return;
  const float inv = 1.0f / l;
  float* const op = p.o + ((long)b * p.Nq + q_row) * p.ldo + (long)head * Dh;
#pragma unroll
  for (int i = 0; i < DT; ++i) {
    const int d = 16 * i + 4 * g;
    if (d < Dh) {
      f32x4 v = acc[i];
#pragma unroll
      for (int r = 0; r < 4; ++r) v[r] *= inv;
      *reinterpret_cast<f32x4*>(op + d) = v;
    }
  }
}

template <int DP>
int launch_attn_x3(crg_ctx* ctx, hipStream_t st, const crg_attn_x3_args& a) {
  const void* kern = reinterpret_cast<const void*>(&attn_x3_kernel<DP>);
  if (int rc = crg_set_dyn_lds(ctx, kern, ax_cfg<DP>::LDS, "attention_x3")) return rc;
  const int vec_v = a.ldvt % 4 == 0 && ((uintptr_t)a.vt & 15) == 0;
  const dim3 grid((a.Nq + AX_ROWS - 1) / AX_ROWS, a.H, a.B);
  hipLaunchKernelGGL((attn_x3_kernel<DP>), grid, dim3(256), ax_cfg<DP>::LDS, st, a, a.scale * 1.4426950408889634f, vec_v);
  CRG_CHECK_LAUNCH(ctx, "attention_x3");
  return 0;
}
}  // namespace

extern "C" int crg_attention_x3(crg_ctx* ctx, void* stream, const crg_attn_x3_args* a) {
  if (!ctx) return -22;
  CRG_REQUIRE(ctx, a && a->q && a->k && a->vt && a->o, "attention_x3: bad arguments");
  CRG_REQUIRE(ctx, a->B > 0 && a->H > 0 && a->Nq > 0 && a->Nk > 0, "attention_x3: empty problem B=%d H=%d Nq=%d Nk=%d", a->B, a->H, a->Nq, a->Nk);
  CRG_REQUIRE(ctx, a->Dh % 8 == 0 && a->Dh >= 8 && a->Dh <= 512, "attention_x3: head dim %d unsupported (multiple of 8, 8 .. 512)", a->Dh);
  CRG_REQUIRE(ctx, a->H <= 65535 && a->B <= 65535, "attention_x3: H=%d / B=%d beyond the grid's 65535", a->H, a->B);
  const int64_t width = (int64_t)a->H * a->Dh;
  CRG_REQUIRE(ctx, a->ldq >= width && a->ldk >= width && a->ldo >= width, "attention_x3: ldq / ldk / ldo must cover H*Dh=%lld", (long long)width);
  CRG_REQUIRE(ctx, a->ldq % 4 == 0 && a->ldk % 4 == 0 && a->ldo % 4 == 0, "attention_x3: ldq / ldk / ldo must keep 16-byte alignment (multiples of 4)");
  CRG_REQUIRE(ctx, a->ldvt >= a->Nk, "attention_x3: ldvt=%lld must cover Nk=%d", (long long)a->ldvt, a->Nk);
  CRG_REQUIRE(ctx, (((uintptr_t)a->q | (uintptr_t)a->k | (uintptr_t)a->o) & 15) == 0 && ((uintptr_t)a->vt & 3) == 0,
              "attention_x3: q, k and o must be 16-byte aligned, vt 4-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  const double flops = 4.0 * a->B * a->H * (double)a->Nq * a->Nk * a->Dh;
  const double bytes = 4.0 * a->B * a->H * a->Dh * (2.0 * a->Nq + 2.0 * a->Nk);
  crg_prof_scope ps(ctx, st, CRG_K_ATTN, flops, bytes);
  if (a->Dh <= 64) return launch_attn_x3<64>(ctx, st, *a);
  if (a->Dh <= 96) return launch_attn_x3<96>(ctx, st, *a);
  if (a->Dh <= 160) return launch_attn_x3<160>(ctx, st, *a);
  if (a->Dh <= 256) return launch_attn_x3<256>(ctx, st, *a);
  return launch_attn_x3<512>(ctx, st, *a);
}
