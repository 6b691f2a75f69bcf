// The planner of crg_attention / crg_attention_v: which kernel a call runs on, as a pure function of the call's sizes, the V layout, the
// heuristic sample count and the four developer knobs.  Host only, plain C++17: no HIP include, no AttnP, no crg_ctx, no getenv.
// attention.hip (attention_entry) validates the call, reads the knobs once per process, asks plan_attention and switches on the plan's
// variant; tools/attn_plan_dump.cpp runs the same function without a device (tests/test_attention_exact_cpu.py).
//
// A new kernel instantiation: a row in CRG_ATTN_VARIANTS, a rule in plan_attention, a case in tests/_attention_exact_cases.py (the CPU
// test holds the union of the cases' plans against this table, row by row).
#pragma once
#include <stdio.h>

namespace crg_attn_plan {

// Kernel families (attention.hip): REG attn_kernel (register-staged), CTX attn_ctx_kernel (few keys, K / V staged once per block),
// DMA attn_dma_kernel (LDS-DMA), SP attn_sp_kernel (software-pipelined LDS-DMA).
enum Family { F_REG = 0, F_CTX, F_DMA, F_SP };
inline const char* family_name(int f) { return f == F_REG ? "reg" : f == F_CTX ? "ctx" : f == F_DMA ? "dma" : "sp"; }

// Every dispatchable variant: X(family, KK, NV, ONES, VRM, NW, OCC, SUB).
//   KK    REG / CTX: KS, 16-wide QK^T k-steps (head dims 16 KS - 8 and 16 KS); DMA / SP: KC, 16-byte chunks of a K row (head dim 8 KC)
//   NV    32-channel blocks of the PV product
//   ONES  a spare V^T row of ones carries the row sum through the PV MFMAs (head dim < 32 NV)
//   VRM   V row-major (crg_attention_v); the LDS-DMA forms take transposed V only
//   NW    waves per block, each on 32 queries;  OCC  the __launch_bounds__ occupancy;  SUB  DMA: the kernel's SUB argument (0 elsewhere)
// The staged kernels' rows: per KS the head dim below 32 NV (ONES), and the one equal to it where 16 KS = 32 NV.
#define CRG_ATTN_STAGED_(X, FAM, VRM) \
  X(FAM, 1, 1, 1, VRM, 4, 3, 0)  \
  X(FAM, 2, 1, 1, VRM, 4, 3, 0) X(FAM, 2, 1, 0, VRM, 4, 3, 0)  \
  X(FAM, 3, 2, 1, VRM, 4, 3, 0)  \
  X(FAM, 4, 2, 1, VRM, 4, 3, 0) X(FAM, 4, 2, 0, VRM, 4, 3, 0)  \
  X(FAM, 5, 3, 1, VRM, 4, 2, 0)  \
  X(FAM, 6, 3, 1, VRM, 4, 2, 0) X(FAM, 6, 3, 0, VRM, 4, 2, 0)  \
  X(FAM, 7, 4, 1, VRM, 4, 1, 0)  \
  X(FAM, 8, 4, 1, VRM, 4, 1, 0) X(FAM, 8, 4, 0, VRM, 4, 1, 0)  \
  X(FAM, 9, 5, 1, VRM, 4, 1, 0)  \
  X(FAM, 10, 5, 1, VRM, 4, 1, 0) X(FAM, 10, 5, 0, VRM, 4, 1, 0)
#define CRG_ATTN_VARIANTS(X) \
  CRG_ATTN_STAGED_(X, CTX, 1) CRG_ATTN_STAGED_(X, CTX, 0)  \
  X(SP, 5, 2, 1, 0, 8, 4, 0) X(SP, 5, 2, 1, 0, 8, 2, 0) X(DMA, 5, 2, 1, 0, 4, 4, 1) X(DMA, 5, 2, 1, 0, 8, 4, 1)  \
  X(SP, 8, 2, 0, 0, 8, 2, 0) X(DMA, 8, 2, 0, 0, 8, 4, 1) X(DMA, 8, 2, 0, 0, 4, 4, 1)  \
  X(SP, 10, 3, 1, 0, 8, 2, 0) X(DMA, 10, 3, 1, 0, 4, 3, 1) X(DMA, 10, 3, 1, 0, 8, 2, 1)  \
  CRG_ATTN_STAGED_(X, REG, 1) CRG_ATTN_STAGED_(X, REG, 0)

struct Variant {
  int family, kk, nv, ones, vrm, nw, occ, sub;
};
#define CRG_ATTN_ROW_(FAM, KK, NV, ONES, VRM, NW, OCC, SUB) {F_##FAM, KK, NV, ONES, VRM, NW, OCC, SUB},
constexpr Variant VARIANTS[] = {CRG_ATTN_VARIANTS(CRG_ATTN_ROW_)};
#undef CRG_ATTN_ROW_
constexpr int N_VARIANTS = (int)(sizeof(VARIANTS) / sizeof(VARIANTS[0]));
// ... and a name per row for the launcher's switch: V_<family>_<KK>_<NV>_<ONES>_<VRM>_<NW>_<OCC>_<SUB> = the row's index in VARIANTS
#define CRG_ATTN_ID_(FAM, KK, NV, ONES, VRM, NW, OCC, SUB) V_##FAM##_##KK##_##NV##_##ONES##_##VRM##_##NW##_##OCC##_##SUB,
enum VariantId { CRG_ATTN_VARIANTS(CRG_ATTN_ID_) V_COUNT };
#undef CRG_ATTN_ID_
static_assert(V_COUNT == N_VARIANTS, "one name per row");

constexpr int find_variant(int family, int kk, int nv, int ones, int vrm, int nw, int occ, int sub) {
  for (int i = 0; i < N_VARIANTS; ++i) {
    const Variant& v = VARIANTS[i];
    if (v.family == family && v.kk == kk && v.nv == nv && v.ones == ones && v.vrm == vrm && v.nw == nw && v.occ == occ && v.sub == sub) return i;
  }
  return -1;
}

// Dev knobs (environment variables, read once per process by attention_entry): names, defaults and meaning as they always were.
struct Knobs {
  int ctx = 1;   // CRG_ATTN_CTX: 0 = the general kernels for few-key shapes too
  int dma = 1;   // CRG_ATTN_DMA: 0 = register-staged kernel only, 1 = software-pipelined where instantiated, else the plain LDS-DMA
                 //   kernel, 8 / 4 = plain LDS-DMA kernel on 8 / 4 waves, 5 = head dim 64 on the software-pipelined kernel
  int tail = 1;  // CRG_ATTN_TAIL: key tails on the LDS-DMA kernel (0: register-staged)
  int occ4 = 1;  // CRG_ATTN_OCC4: head dim 40, software-pipelined: four blocks per CU (0: two)
};

struct Plan {
  int rc = 0;  // 0, or the error code with its message
  char msg[160] = {0};
  int variant = -1;  // index into VARIANTS
  unsigned grid_x = 0, grid_y = 0, threads = 0;
};

inline Plan refuse(const char* what, int v) {
  Plan pl;
  pl.rc = -22;
  snprintf(pl.msg, sizeof pl.msg, what, v);
  return pl;
}

// ldk / ldv in elements (ldv: the row stride of V^T, or of row-major V when vrm); heur_samples: the batch that the size heuristics
// read - B itself, or the batch-invariant mode's sample count (crg_heur_samples), so that no decision depends on how many samples
// share the launch.
inline Plan plan_attention(int B, int H, int Nq, int Nk, int Dh, long ldk, long ldv, bool vrm, long heur_samples, const Knobs& kn) {
  if (B <= 0 || H <= 0 || Nq <= 0 || Nk <= 0) return refuse("attention: empty problem (Nk = %d)", Nk);
  if (Dh % 8 != 0 || Dh < 8 || Dh > 160) return refuse("attention: head dim %d unsupported", Dh);
  Plan pl;
  const int ks = (Dh + 15) / 16, nv = (ks + 1) / 2;
  const int nqg = (Nq + 127) / 128, bh = B * H;
  const int staged_occ = ks <= 4 ? 3 : (ks <= 6 ? 2 : 1);
  pl.grid_y = (unsigned)bh;
  // few keys (cross-attention against the prompt context, FaceID tokens, 8x8 self-attention): K / V staged once per block, no barrier in
  // the loop ... used where a block then walks at least two query groups behind one staging of the keys (measured, kernel trace: 8 x 4096
  // queries x 77 keys, d 40: 22.3 -> 19.6 us; with ONE group per block - 1024 queries, d 80 - the general kernel's interior-tile
  // staging is the faster one, 12.6 vs 13.5 us).  These launches are bound by their 80-byte-per-head Q / O row slices (32 cache
  // lines per wave-instruction), not by block count: see DESIGN 4.
  // (batch-invariant mode: the block count of heur_samples samples - the two kernels sum the keys in different orders)
  if (kn.ctx && Nk <= 128 && (long)nqg * heur_samples * H >= 2048) {
    // blocks per (batch, head): the largest divisor of the 128-query group count that keeps the grid within four blocks per CU,
    // so that every block walks the same number of groups behind ONE staging of the key tiles
    int gx = 1;
    for (int d = 1; d <= nqg; ++d)
      if (nqg % d == 0 && (long)d * bh <= 1024) gx = d;
    pl.variant = find_variant(F_CTX, ks, nv, Dh < nv * 32, vrm, 4, staged_occ, 0);
    pl.grid_x = (unsigned)gx;
    pl.threads = 256;
    return pl;
  }
  // LDS-DMA forms: transposed V, whole 64-key tiles (or a masked key tail), extents addressable through a 32-bit buffer descriptor
  if (kn.dma && !vrm && (Nk % 64 == 0 || (kn.tail && Nk > 8)) && ((long)Nk * ldk * 2 < (1l << 31)) && ((long)Dh * ldv * 2 < (1l << 31)) &&
      (Dh == 40 || Dh == 64 || Dh == 80)) {
    const bool sp = kn.dma == 1 && Nk % 128 == 0;
    int fam = F_DMA, nw = 4, occ = 4, sub = 1;
    if (Dh == 40) {
      // few key tiles (cross-attention: 77 keys): 128-query blocks, i.e. twice the blocks and four-wave barriers (19.2 vs 19.9 us)
      if (sp) fam = F_SP, nw = 8, occ = kn.occ4 ? 4 : 2, sub = 0;
      else nw = (kn.dma == 4 || (kn.dma == 1 && Nk <= 256)) ? 4 : 8;
    } else if (Dh == 64) {  // measured (B4 N4096 h10: register-staged 256 us, pipelined 253, LDS-DMA on 8 waves 233, on 4 waves 226): plain form, 4 waves
      if (kn.dma == 5 && Nk % 128 == 0) fam = F_SP, nw = 8, occ = 2, sub = 0;
      else nw = kn.dma == 8 ? 8 : 4;
    } else {
      if (sp) fam = F_SP, nw = 8, occ = 2, sub = 0;
      else if (kn.dma == 4) nw = 4, occ = 3;
      else nw = 8, occ = 2;
    }
    const int kc = Dh / 8, dnv = (Dh + 31) / 32;
    pl.variant = find_variant(fam, kc, dnv, kc * 8 < dnv * 32, 0, nw, occ, sub);
    pl.grid_x = (unsigned)((Nq + 32 * nw - 1) / (32 * nw));
    pl.threads = 64u * nw;
    return pl;
  }
  pl.variant = find_variant(F_REG, ks, nv, Dh < nv * 32, vrm, 4, staged_occ, 0);
  pl.grid_x = (unsigned)nqg;
  pl.threads = 256;
  return pl;
}

}  // namespace crg_attn_plan
