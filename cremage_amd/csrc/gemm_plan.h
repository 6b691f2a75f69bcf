// The planner of crg_gemm / crg_conv2d: every size decision of the GEMM / conv dispatcher as a pure function of the call's arguments
// and a small environment - tile width, configuration A / C / D, split-K factor, tail split, row-halo form, the staggered 256-pixel
// kernel, the persistent ring GEMM, paired epilogue, XCD partition, the reduce kernel that follows and the GroupNorm statistics
// granularity.  Host only, plain C++17: no HIP include, no GemmP, no crg_ctx, no getenv.  Pointers are read for null-ness and 16-byte
// alignment, never dereferenced.  gemm_conv.hip (the launcher) fills GemmP from the args and the plan, asks the planned family's
// picker (one per kernel file, gemm_shared.h) for the kernel pointer and launches; tools/plan_dump.cpp runs the same functions without a device (tests/test_gemm_plan_cpu.py).
//
// A new route: a rule here, a case in that kernel family's picker (pick_* in the family's own file), rows in tests/routes/ (DESIGN.md section 4).
#pragma once
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/crg_hip.h"

namespace crg_plan {

constexpr int BK = 64;  // k-tile (gemm_shared.h: crg_mm::BK)
#ifndef CRG_C_STAGES  // dev knob (tools/build_one_variant.sh): ring depth of configuration C
#define CRG_C_STAGES 4
#endif

// Dev knobs (environment variables CRG_*; read once by the launcher, crg_mm::plan_env): names, defaults and meaning as they always were.
struct Knobs {
  int split_blocks = 512;  // CRG_SPLIT_BLOCKS: blocks aimed at by the K cut
  int split_max = 16;      // CRG_SPLIT_MAX: most K slices
  int gemm_cfg = 0;        // CRG_GEMM_CFG: force a configuration, 1 = A, 3 = C, 4 = D
  int d_max = 384;         // CRG_GEMM_D_MAX: 64-row tiles below this many 128-row tiles (plain epilogues)
  int d_max_g = 384;       // CRG_GEMM_D_MAXG: ... GEGLU epilogues (3x3 convs keep it: above it they run on the row-halo / ring kernels)
  int d_max_c1 = 384;      // CRG_CONV1_D_MAX: ... 1x1 convs (virtual-concat skip convs)
  bool rowhalo_set = false;  // CRG_ROWHALO: 0 plain implicit GEMM, 1 128-row tiles only, 2 256-row tiles as well; unset: 2 on the half
  int rowhalo = 0;           //   path, 1 on the pre-split-planes path (which has no 256-row form)
  int gemm_ring = 1;        // CRG_GEMM_RING: 0 = never, 1 = GEGLU GEMMs with >= 3 tiles per CU, 2 = plain epilogues as well
  int gemm_ring_min = 300;  // CRG_GEMM_RING_MIN: least tiles of the ring GEMM, % of the CU count
  int gemm_ring_super = 1;  // CRG_GEMM_RING_SUPER (launch_gemm_ring, A/B): 0 = n-fastest tile order inside an XCD's share
  int gemm_ring_stag = 1;   // CRG_GEMM_RING_STAG (launch_gemm_ring): 0 = all eight waves in lockstep
};

struct Env {
  int tune_samples = 0;  // batch-invariant mode (crg_ctx_set_invariant): 0 = off, else the sample count every size heuristic reads
  int n_cu = 0;          // compute units of the device (0 = unknown: 256)
  Knobs knobs;
};

enum Family { F_NONE = 0, F_GEMM_REG, F_GLDS, F_ROWHALO, F_CONV_PP, F_GEMM_RING };

// One kernel launch: the kernel family and its template selectors, the launch geometry, and the per-launch fields of GemmP.
struct Launch {
  int family = F_NONE;
  // selectors.  F_GEMM_REG: wnt, ns (k-groups = split planes), a_f32, y_f32.  F_GLDS: wnt, y_f32, cfg (1 = A, 3 = C, 4 = D), ns (2 = pre-split
  // planes), pair, xt (epilogue extra: 1 GroupNorm statistics, 2 LayerNorm row statistics, 3 LayerNorm correction).  F_ROWHALO: wnt, y_f32,
  // pair, ns, mt (256-row tiles: 2), mx, taps (sub-pixel form: 2).  F_CONV_PP, F_GEMM_RING: wnt.  `conv` is the entry point's.
  int wnt = 0, ns = 1, cfg = 1, a_f32 = 0, y_f32 = 0, xt = 0, mt = 1, mx = 0, taps = 3;
  unsigned grid_x = 0, grid_y = 1, threads = 0;
  size_t lds = 0, lds_cap = 0;  // dynamic LDS bytes of this launch, and the limit to raise the kernel's attribute to
  int splits = 1, ks_q = 0, ks_r = 0;  // K slices; units (k-tiles, or row-halo groups) per slice: units = splits * ks_q + ks_r
  int tile_base = 0, tile_count = 0, slab_row0 = 0;
  int pair = 0;
};

struct Plan {
  int rc = 0;  // 0, or the error code with its message
  char msg[400] = {0};
  Launch main, tail;  // tail.family == F_NONE: no tail launch
  int reduce = CRG_REDUCE_NONE;  // the launch that sums the K slices of the last launch (enum crg_route_reduce)
  int reduce_vpt = 0;            // CRG_REDUCE_GN: values per thread (template selector)
  unsigned reduce_gx = 0, reduce_gy = 1;
  size_t scratch_bytes = 0;  // the split-K slab (of the tail launch, when there is one)
  // GemmP fields of the whole call
  int tiles_n = 0, tiles_m = 0, xg_m = 1, xg_n = 1, xg_s = 0;
  int rowhalo = 0, halo_lin = 0, ring = 0, cm = 0;
  unsigned a_bytes = 0, x2_bytes = 0, w_bytes = 0;
  int gstat_rows = 32;
  bool gn_fused = false;  // the reduce also runs the GroupNorm behind the conv (crg_conv_args.gn_y): no crg_groupnorm to follow
  crg_route route = {};
};

// ---- the rules that used to be written out in several places ----
// 160-wide tiles when they divide N (all UNet widths are multiples of 320), else 128-wide; GEGLU epilogues take 128
inline int wide_wnt(int N, bool geglu) { return (!geglu && N % 160 == 0) ? 5 : 4; }
// ... and 32-wide tiles for conv_out-like thin outputs
inline int tile_wnt(int N, bool geglu) { return (!geglu && N <= 32) ? 1 : wide_wnt(N, geglu); }

// The conv as a GEMM - rows, K (= the packed weight's row length) and the row stride of the per-sample channel vector: the launcher fills
// GemmP from the same three functions.  Sub-pixel form: per parity 2 x 2 taps; the four [Cout][4 Cin] slabs follow each other.
inline int conv_rows(const crg_conv_args& a) { return a.N * a.Ho * a.Wo; }
inline int conv_k(const crg_conv_args& a) { return (a.upsample2x == 2 ? 4 : a.ksize * a.ksize) * (a.C1 + a.C2); }
inline long conv_cvec_ld(const crg_conv_args& a) { return a.cvec_ld ? a.cvec_ld : a.Cout; }

// The call as the decisions read it.
struct Prob {
  bool conv = false;
  int M = 0, N = 0, K = 0, batch = 1, epi = 0, bias_mode = 0, a_dtype = 0, y_dtype = 0, prec = 0, a_is_weight = 0;
  long lda = 0, ldw = 0, ldy = 0, y_bs = 0, ldr = 0, r_bs = 0, cvec_ld = 0;
  bool a_lo = false, w_lo = false, bias = false, res = false, cvec = false, gstat = false, vt = false, rstat = false, ln_stat = false;
  bool y_al16 = true, res_al16 = true, bias_al16 = true, ln_s_al16 = true;
  int rstat_parts = 0;
  // conv geometry
  int C2 = 0, H = 0, W = 0, Ho = 0, Wo = 0, ks = 0, up = 0, mx = 0;
  int cm = 0, rowhalo = 0, halo_lin = 0;  // rowhalo: eligible for conv3_rowhalo_kernel
  unsigned a_bytes = 0, x2_bytes = 0, w_bytes = 0;
  bool gstat_tile_ok = false, gn_y = false, gn_gamma = false, gn_beta = false;
  int gn_groups = 0, gn_hw = 0;
  // what the size heuristics read: the call's own rows and batch, or - batch-invariant mode - tune_samples samples of the per-sample
  // problem (rps = rows per sample then, else 0), so that no decision depends on how many samples share the launch
  long hM = 0;
  int hbatch = 1, hrps = 0;
  double a_foot = 0, w_foot = 0;  // operand footprints in bytes (XCD partition)
};

inline bool al16(const void* p) { return ((uintptr_t)p & 15) == 0; }

inline void fail(Plan& pl, int rc, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(pl.msg, sizeof(pl.msg), fmt, ap);
  va_end(ap);
  pl.rc = rc;
}

inline void set_heur(Prob& q, const Env& e, long M, int batch, int rps, bool samples_along_batch) {
  q.hM = M; q.hbatch = batch; q.hrps = 0;
  if (e.tune_samples <= 0) return;
  if (samples_along_batch) q.hbatch = e.tune_samples;
  else { q.hM = (long)e.tune_samples * rps; q.hrps = rps; }
}

// Blocks of `rows`-row tiles the size heuristics count.  The launch itself always covers the real M.
inline long heur_blocks(const Prob& q, int tiles_n, int rows) { return (long)tiles_n * ((q.hM + rows - 1) / rows) * q.hbatch; }

// Split-K factor: small-M problems (8x8 / 16x16 UNet levels, token GEMMs with few rows) launch far fewer than 2 blocks per CU and stream
// long K; cut K so that ~512 blocks are in flight, keeping >= 8 k-tiles per slice.  Costs one fp32 slab round trip + one extra launch, so
// only when the tile count is low.
inline int choose_splits(const Prob& q, const Knobs& k, long blocks) {
  if (q.epi == CRG_EPI_GEGLU || (q.N & 3) || q.ln_stat) return 1;  // (the LayerNorm correction is per whole row sum: no K slices)
  const int nk = (q.K + BK - 1) / BK;
  // 256..511 blocks leave one block (4 waves) on most CUs, which hides neither the barrier nor the DMA latency: cut K in two when it is
  // long enough to amortise the slab pass (measured: 8x32x32 640->640 conv 112 -> 89 us, 1280->640 203 -> 137 us; K = 2560 GEMMs lose
  // 5 %, hence the nk bound).  Short K (nk < 24) is not split: measured slower than the 64-row / 8-wave configuration on the unsplit
  // problem (128..255 tiles with a K of 24..63 k-tiles - the 16x16-level 1x1 skip convs over a concat, 2048 x 1280 x 1920 / 2560 - are
  // faster unsplit on the 64-row / 8-wave configuration: 30.3 -> 24.0 us and 33.6 -> 30.5 us, tools/c1_probe.py)
  if (blocks >= 512 || nk < 24 || (blocks >= 128 && nk < 64)) return 1;
  if (blocks >= 256) {
    // one to two blocks per CU and a long K: among 2..4 slices take the one whose blocks fill whole rounds of 512 best
    // (256 tiles -> 2, 288 tiles (768x768 latents at the 48x48 level) -> 3, 384 -> 4); ties go to fewer slices
    int s = 2;
    double best = 1e9;
    for (int c = 2; c <= 4; ++c) {
      const double t = (double)((blocks * c + 511) / 512) / c;
      if (t < best - 1e-9) {
        best = t;
        s = c;
      }
    }
    return s;
  }
  int s = (int)((k.split_blocks + blocks - 1) / blocks);
  if (s > nk / 8) s = nk / 8;
  if (s > k.split_max) s = k.split_max;
  return s < 2 ? 1 : s;
}

// Shapes the persistent ring kernel (gemm_ring.hip) takes in place of gemm_glds_kernel: bf16 in / out, one problem (no batch), K a
// multiple of 64, plain or GEGLU epilogue (no SiLU, no per-row bias, no timestep vector, no GroupNorm statistics), the weight
// addressable through a 32-bit buffer descriptor - and, by measurement (tools/lin_probe.py / lin_probe_xl.py, device time inside a
// captured graph):
//   GEGLU epilogue, >= 3 tiles per CU : 8192 x 5120 x 640   82 -> 71 us,  16384 x 5120 x 640  164 -> 145 us,  4096 x 10240 x 1280  139 -> 127 us
//   GEGLU, 2.5 tiles per CU           : 2048 x 10240 x 1280  69 -> 69 us (equal)
//   plain epilogue (any tile count)   : 32768 x 320 x 320 + residual 18.6 -> 21.9 us, 8192 x 1920 x 640 30.5 -> 34.4 us, 32768 x 320 x 1280
//                                       36 -> 40 us, 16384 x 1920 x 640 58.5 -> 57 us: the two-blocks-per-CU kernel hides its short epilogue
//                                       behind the other block's MFMAs already; this kernel's 52 one-KiB DMA pieces per k-tile (the row-halo
//                                       conv needs 32) then cost more issue time than the larger tile saves
// so it is routed for GEGLU GEMMs with at least three 256-row tiles per CU (knobs gemm_ring / gemm_ring_min).  The tile count is taken
// from the heuristics' rows: under the batch-invariant mode the kernel is then also launched on fewer tiles than CUs.
inline bool ring_gemm_ok(const Prob& q, int splits, const Env& e) {
  const int on = e.knobs.gemm_ring;
  if (!on || q.batch != 1 || q.K % 64 || q.K < 128 || splits != 1) return false;
  if (q.epi != CRG_EPI_GEGLU && !(on >= 2 && q.epi == CRG_EPI_NONE)) return false;
  if (q.bias_mode == CRG_BIAS_ROW || q.cvec || q.gstat || q.vt || q.rstat) return false;
  if (q.ln_stat && (q.res || !q.ln_s_al16)) return false;
  const bool geglu = q.epi == CRG_EPI_GEGLU;
  if (geglu ? (q.N % 32 || (q.ldy & 3)) : (q.N % 8 || (q.ldy & 7) || !q.y_al16)) return false;
  if (q.res && ((q.ldr & 7) || !q.res_al16)) return false;
  if (q.bias && !q.bias_al16) return false;
  if ((double)q.N * q.ldw * 2 >= 2147483648.0) return false;
  const int bn = 32 * wide_wnt(q.N, geglu);
  const long tiles = ((q.hM + 255) / 256) * ((q.N + bn - 1) / bn);
  return tiles * 100 >= (long)(e.n_cu > 0 ? e.n_cu : 256) * e.knobs.gemm_ring_min;
}

// ... and every extent that grows with the rows of the CALL addressable through a 32-bit buffer descriptor
inline bool ring_gemm_fits(const Prob& q) {
  const double lim = 2147483648.0;
  return !((double)q.M * q.lda * 2 >= lim || (double)q.M * q.ldy * 2 >= lim || (q.res && (double)q.M * q.ldr * 2 >= lim));
}

// (xg_m, xg_n, xg_s): see block_to_tile.  Minimise fabric traffic xg_n*|A| + xg_m*|W| over the feasible factorizations of 8.
inline void choose_xcd_partition(const Prob& q, int splits, Plan& pl) {
  pl.xg_m = pl.xg_n = 1;
  pl.xg_s = 0;
  double best = 0.0;
  for (int gs = 8; gs >= 1; gs >>= 1) {
    if (splits % gs) continue;
    for (int gn = 1; gn * gs <= 8; gn <<= 1) {
      const int gm = 8 / (gs * gn);
      if (pl.tiles_n % gn || pl.tiles_m % gm) continue;
      const double cost = gn * q.a_foot + gm * q.w_foot;
      if (!pl.xg_s || cost < best) {
        best = cost;
        pl.xg_m = gm; pl.xg_n = gn; pl.xg_s = gs;
      }
    }
  }
}

// K slices of the row-halo kernels are (chunk, kernel row) groups: three k-tiles, two in the sub-pixel form
// CRG_ROWHALO with the path's default: 2 on the half path, 1 on pre-split planes (which have no 256-row form)
inline int rowhalo_knob(const Knobs& k, bool planes) { return k.rowhalo_set ? k.rowhalo : (planes ? 1 : 2); }

inline int halo_groups(const Prob& q) { return (q.K / BK) / (q.up == 2 ? 2 : 3); }

// Does the row-halo kernel run?  knob: CRG_ROWHALO with the path's default; the sub-pixel form exists on this kernel only (no knob).
inline bool halo_runs(const Prob& q, int knob, int splits) {
  return (knob || q.up == 2) && q.rowhalo && q.batch == 1 && splits <= halo_groups(q);
}

// dynamic LDS of a row-halo launch: `ns` weight planes, double-buffered, and as many row buffers of XP one-KiB pieces for TP-pixel tiles
inline size_t halo_lds(const Prob& q, int wnt, int ns, int TP) {
  const int Wg = q.up == 2 ? q.W : q.Wo;  // (sub-pixel form: geometry of the source grid)
  const int XP = (q.halo_lin || Wg > TP) ? (TP + 2 + 7) / 8 : ((TP / Wg) * (Wg + 2) + 7) / 8;
  return (size_t)ns * ((size_t)2 * 32 * wnt * 128 + (size_t)2 * XP * 1024);
}

enum Path { P_HALF, P_REG_X3, P_PLANES };  // one 16-bit plane (fp32 A: register-staged) | fp32-class on unsplit operands | on pre-split planes

inline void set_route(Plan& pl, const Prob& q, const Launch& L, Path path) {
  crg_route& r = pl.route;
  const bool halo = L.family == F_ROWHALO || L.family == F_CONV_PP;
  r = crg_route{};
  r.wnt = L.wnt;
  r.splits = L.splits;
  r.halo_lin = halo ? q.halo_lin : 0;
  r.up2 = q.up == 2 ? 1 : 0;
  r.gn_stats_rows = q.gstat ? pl.gstat_rows : 0;
  if (path == P_PLANES) {
    r.kernel = CRG_ROUTE_PLANES;
    r.rowhalo = halo ? 1 : 0;
    r.mx = q.mx ? 1 : 0;
    return;
  }
  r.kernel = L.family == F_CONV_PP ? CRG_ROUTE_CONV_PP : halo ? CRG_ROUTE_ROWHALO : L.family == F_GLDS ? CRG_ROUTE_GLDS : CRG_ROUTE_GEMM_REG;
  r.config = L.family == F_GEMM_REG ? 0 : L.cfg;
  r.rowhalo = halo ? pl.rowhalo : 0;
  r.pair = L.pair;
}

// One launch of the tile range and K cut that L holds on entry (splits, tile_base, tile_count, slab_row0): kernel, epilogue, geometry.
// cfg: 1 = A (128 x BN tile, 4 waves, 2-deep ring), 3 = C, 4 = D (see plan_launches).  Sets pl.route to this launch's record.
inline bool plan_kernel(const Prob& q, const Env& e, Path path, int wnt, int cfg, bool a_f32, Launch& L, Plan& pl) {
  const int BN = 32 * wnt;
  const bool y_f32 = q.y_dtype == CRG_F32, glds = path == P_HALF && !a_f32, planes = path == P_PLANES;
  int units = (q.K + BK - 1) / BK;  // K slices in k-tiles ...
  L.wnt = wnt; L.cfg = cfg; L.a_f32 = a_f32; L.y_f32 = y_f32; L.grid_y = q.batch;
  L.pair = (glds && !y_f32 && L.splits == 1 && q.epi != CRG_EPI_GEGLU && (q.N & 7) == 0 && (q.ldy & 7) == 0 && (q.y_bs & 7) == 0 && q.y_al16 &&
            (!q.res || ((q.ldr & 7) == 0 && (q.r_bs & 7) == 0 && q.res_al16)) && (!q.cvec || (q.cvec_ld & 3) == 0)) ? 1 : 0;
  if (!planes) {
    if (q.vt && !(L.pair && L.splits == 1 && !q.gstat && !q.conv))
      return fail(pl, -22, "gemm: a transposed column range needs the paired bf16 epilogue of an unsplit, unbatched GEMM (N, ldy multiples of 8, K below the split-K rule)"), false;
    if (q.gstat && !L.pair && L.splits == 1)
      return fail(pl, -22, "gemm/conv: GroupNorm statistics come from the paired bf16 epilogue (N, ldy, ldr multiples of 8, 16-byte aligned y / residual, no GEGLU)"), false;
    if (q.rstat && !(!q.gstat && !q.vt && !q.conv && q.batch == 1 && !y_f32 && q.rstat_parts == 2 * pl.tiles_n && q.epi == CRG_EPI_NONE &&
                     ((L.splits == 1 && L.pair) || (L.splits > 1 && (q.N & 3) == 0 && (q.ldy & 3) == 0 && (!q.res || (q.ldr & 3) == 0)))))
      return fail(pl, -22, "gemm: LayerNorm row statistics come from the paired bf16 epilogue of an unbatched plain GEMM (N, ldy multiples of 8) or from its split-K reduce, with row_stats_parts = 2 * ceil(N / tile) = %d (got %d)", 2 * pl.tiles_n, q.rstat_parts), false;
    if (q.ln_stat && !(glds && !y_f32 && !q.conv && L.splits == 1 && q.batch == 1 && !q.res && !q.gstat && !q.rstat && !q.cvec && (q.N & 3) == 0 &&
                       (q.bias_mode == CRG_BIAS_COL || q.bias_mode == CRG_BIAS_NONE) && (q.epi == CRG_EPI_NONE || q.epi == CRG_EPI_GEGLU)))
      return fail(pl, -22, "gemm: the LayerNorm epilogue needs an unsplit, unbatched bf16 GEMM (N %% 4 == 0) without residual / statistics / SiLU"), false;
  }
  if (glds || planes) {
    // LDS-DMA kernel: NS planes x STAGES x (A tile + W tile) + the dummy-load target.  Pre-split planes: the 128 x BN tile on 8 waves in two
    // k-groups, 2-deep ring (4 planes x 2 stages fill the LDS: one block per CU, so the second wave per SIMD comes from the k-groups)
    const int ns = planes ? 2 : 1, stages = cfg == 3 ? CRG_C_STAGES : 2, wmt = cfg == 1 ? 4 : 2, kg = (planes || cfg == 3) ? 2 : 1;
    L.family = F_GLDS; L.ns = ns; L.threads = 256 * kg;
    L.lds = L.lds_cap = (size_t)ns * stages * (32 * wmt + BN) * 128 + 1024;
    if (!y_f32 && !q.conv && q.ln_stat) L.xt = 3;
    else if (!y_f32 && !q.conv && q.rstat && L.splits == 1) L.xt = 2;
    else if (L.pair && q.gstat && L.splits == 1) L.xt = 1;
  } else {  // register-staged operands: split-bf16 runs 8 waves (two k-groups)
    const int ns = path == P_REG_X3 ? 2 : 1;
    L.family = F_GEMM_REG; L.ns = ns; L.threads = 256 * ns;
    L.lds = L.lds_cap = (size_t)2 * ns * (128 + BN) * 128;
  }
  // the row-halo kernel takes configuration A's place (3x3 / stride 1 / pad 1, chunk-major K, tiles of 128 or more columns)
  if (q.conv && (wnt == 4 || wnt == 5) && (planes || (glds && cfg == 1 && !y_f32))) {
    const int knob = rowhalo_knob(e.knobs, planes);
    if (halo_runs(q, knob, L.splits)) {
      const int form = planes ? 1 : pl.rowhalo;
      L.family = F_ROWHALO; L.xt = 0;
      L.ns = planes ? 2 : 1; L.mt = form == 2 ? 2 : 1; L.mx = q.mx; L.taps = q.up == 2 ? 2 : 3;
      L.threads = 256 * L.ns * L.mt;
      L.lds = halo_lds(q, wnt, L.ns, form == 2 ? 256 : 128);
      // (planes: eligible widths need <= 18 pieces per row buffer)
      L.lds_cap = planes ? (size_t)(2 * 2 * BN * 128 + 2 * 2 * 18 * 1024) : (size_t)(form == 2 ? 116 : 80) * 1024;
      units = halo_groups(q);  // ... or in (chunk, kernel row) groups
    }
  }
  if (q.up == 2 && L.family != F_ROWHALO)
    return fail(pl, -22, planes ? "conv2d: the sub-pixel upsample form runs on the row-halo kernel only (Cout > 32)"
                                : "conv2d: the sub-pixel upsample form runs on the row-halo kernel only (Cout > 32, bf16 output or split planes)"), false;
  if (planes && q.mx && L.family != F_ROWHALO)
    return fail(pl, -22, "conv2d: the MX form takes 3x3 / stride 1 / pad 1 convs with Cin %% 64 == 0 (the row-halo kernel's domain)"), false;
  L.ks_q = units / L.splits;
  L.ks_r = units % L.splits;
  L.grid_x = (unsigned)(L.tile_count * L.splits);
  if (L.family == F_ROWHALO && !planes && pl.rowhalo == 2 && pl.ring) {
    // the staggered 256-pixel-tile kernel (conv_pp.hip).  One statistics partial per tile and channel instead of eight (crg_groupnorm_pre
    // then needs no finalise launch): paired epilogue, no K slices, tiles that do not straddle samples
    L.family = F_CONV_PP;
    if (q.gstat && q.gstat_tile_ok && L.pair && L.splits == 1 && (q.Ho * q.Wo) % 256 == 0) pl.gstat_rows = 256;
  }
  set_route(pl, q, L, path);
  return true;
}

// can the reduce behind this split-K launch also run the GroupNorm the caller asked for?
inline bool gn_slab_ok(const Prob& q, const Launch& L) {
  if (q.y_dtype == CRG_F32 || !q.gn_y || !q.gn_gamma || !q.gn_beta || q.batch != 1 || L.slab_row0 != 0 || q.gstat || q.vt || q.rstat) return false;
  if (q.epi != CRG_EPI_NONE || (q.bias_mode != CRG_BIAS_NONE && q.bias_mode != CRG_BIAS_COL)) return false;
  if (q.gn_groups <= 0 || q.N % q.gn_groups || q.gn_hw <= 0 || q.M % q.gn_hw || q.ldy != q.N) return false;
  const int gs = q.N / q.gn_groups;
  if (gs % 8 || (q.N & 7) || (q.res && (q.ldr & 7)) || (q.cvec && (q.cvec_ld & 3))) return false;
  return (long)q.gn_hw * (gs >> 3) <= 256 * 8;
}

// the reduce launch behind a split-K launch (whole problem, or - tail split - the rows >= slab_row0)
inline bool plan_reduce(const Prob& q, const Launch& L, Plan& pl) {
  const long rows = q.M - L.slab_row0;
  const bool y_f32 = q.y_dtype == CRG_F32;
  if (gn_slab_ok(q, L)) {
    pl.reduce = CRG_REDUCE_GN;
    pl.reduce_vpt = (int)(((long)q.gn_hw * (q.N / q.gn_groups >> 3) + 255) / 256);
    pl.reduce_gx = q.gn_groups; pl.reduce_gy = q.M / q.gn_hw;
    pl.gn_fused = true;
  } else if (q.rstat) {
    if (y_f32 || q.batch != 1 || (q.N & 3) || (q.ldy & 3) || q.epi != CRG_EPI_NONE || q.cvec || q.rstat_parts > 64 || (q.res && (q.ldr & 3)))
      return fail(pl, -22, "gemm: LayerNorm row statistics behind split-K need an unbatched plain bf16 problem with 4-aligned N / ldy / ldr"), false;
    const long blocks = (rows + 3) / 4;
    pl.reduce = CRG_REDUCE_ROWS;
    pl.reduce_gx = (unsigned)(blocks > 4096 ? 4096 : blocks);
  } else if (q.gstat) {
    if (q.batch != 1 || (q.N & 3) || (q.ldy & 3) || (L.slab_row0 & 31) || (q.res && (q.ldr & 3)))
      return fail(pl, -22, "gemm: GroupNorm statistics need an unbatched problem with 4-aligned N / ldy / ldr"), false;
    pl.reduce = CRG_REDUCE_STATS;
    pl.reduce_gx = (unsigned)((rows + 31) / 32); pl.reduce_gy = (unsigned)((q.N + 127) / 128);
  } else {
    const long total4 = rows * (q.N >> 2);
    pl.reduce = CRG_REDUCE_PLAIN;
    pl.reduce_gx = (unsigned)((total4 + 255) / 256 > 2048 ? 2048 : (total4 + 255) / 256); pl.reduce_gy = q.batch;
  }
  pl.route.reduce = pl.reduce;
  return true;
}

// Tile / pipeline configuration of the LDS-DMA kernel, by how many blocks the problem yields (256 CUs):
//   A  128 x BN tile, 4 waves, 2-deep ring  : >= ~1.5 blocks per CU (after split-K); two blocks share a CU and hide each
//                                             other's latencies
//   D   64 x BN tile, 4 waves, 2-deep ring  : 192..1023 tiles of 128 rows (GEGLU epilogues: 192..383) and a short K: twice the blocks
//                                             (4096x1280x1280: A 26.7, 8-wave 128-row variant 25.5, D 23.6 us).  Device time inside a
//                                             captured graph (tools/lin_probe.py): 32768x320x320 + residual 25.8 (A) -> 22.4,
//                                             8192x1920x640 41.6 -> 35.3, 2048x3840x1280 41.8 -> 34.6, 32768x320x1280 49.8 -> 45.3 us; the
//                                             GEGLU GEMMs (128-wide tiles, heavy epilogue) keep A: 8192x5120x640 82 (A) vs 89 (D)
//   C   64 x BN tile, 8 waves (two k-groups, folded through LDS), 4-deep ring : < 192 tiles (16x16 / 8x8 token GEMMs): one
//                                             block per CU at most, so the waves and the ring depth come from inside the block
//                                             (2048x1280x1280: A 24.7, C 16.7 us)
// Pre-split planes (P_PLANES) have one configuration and no 256-row form, ring kernel or tail split.
inline void plan_launches(const Prob& q, const Env& e, Path path, int wnt, bool a_f32, Plan& pl) {
  const Knobs& k = e.knobs;
  const int BN = 32 * wnt;
  const bool y_f32 = q.y_dtype == CRG_F32, glds = path == P_HALF && !a_f32, planes = path == P_PLANES;
  const bool inv = e.tune_samples > 0;  // batch-invariant mode: every size below is that of tune_samples samples (heur_blocks)
  const bool halo2_kernels = glds && q.conv && !y_f32 && (wnt == 4 || wnt == 5);  // the 256-row forms exist for these
  if (planes && q.gstat && (q.batch != 1 || (q.N & 3) || (q.M & 31) || (q.ldy & 3)))
    return fail(pl, -22, "gemm/conv: GroupNorm statistics need an unbatched problem with N %% 4 == 0 and M %% 32 == 0");
  pl.tiles_n = (q.N + BN - 1) / BN;
  // split-K first, on 128-row tiles: a long K is the cheapest source of blocks.  Only problems that stay below ~1 block per
  // CU after that (short K) change the tile / wave configuration.
  pl.tiles_m = (q.M + 127) / 128;
  Launch& L = pl.main;
  // (planes with statistics: they come out of the epilogue, so no K split)
  L.splits = (planes && q.gstat) ? 1 : choose_splits(q, k, heur_blocks(q, pl.tiles_n, 128));
  if (glds && !q.conv && !y_f32) {
    // persistent 256-row tiles (gemm_ring.hip) where every CU gets at least (almost) one: more FLOP per staged byte, no per-tile prologue
    // (batch-invariant mode, a_is_weight: `batch` is the sample count, which ring_gemm_ok reads - knob gemm_ring = 2 only, since the
    // default rule takes GEGLU GEMMs alone - so those calls stay on the kernel below whatever their batch)
    if (!(inv && q.a_is_weight) && ring_gemm_ok(q, L.splits, e)) {
      if (ring_gemm_fits(q)) {
        L.family = F_GEMM_RING;
        L.wnt = wide_wnt(q.N, q.epi == CRG_EPI_GEGLU);
        pl.route = crg_route{};
        pl.route.kernel = CRG_ROUTE_GEMM_RING;
        pl.route.wnt = L.wnt;
        pl.route.splits = 1;
        return;
      }
      // (mode off: the two-blocks-per-CU kernel takes what the descriptors cannot address.  Under the mode that would be a route picked by
      // the size of the call)
      if (inv) return fail(pl, -22, "gemm: batch-invariant mode routes this problem to the persistent 256-row kernel, whose 32-bit buffer descriptors cannot address M=%d rows: split the call", q.M);
    }
  }
  int cfg = 1;
  if (glds && L.splits == 1) {
    const long blocks = heur_blocks(q, pl.tiles_n, 128);
    if (blocks < 192) cfg = 3;
    else if (blocks < (q.conv ? (q.ks == 1 ? k.d_max_c1 : k.d_max_g) : (q.epi == CRG_EPI_GEGLU ? k.d_max_g : k.d_max))) cfg = 4;
  }
  if (glds && k.gemm_cfg) cfg = k.gemm_cfg;
  if (q.up == 2) cfg = 1;  // the sub-pixel upsample form exists on the row-halo kernel (configuration A's place) only
  if (cfg == 3 || cfg == 4) {
    pl.tiles_m = (q.M + 63) / 64;
    L.splits = k.gemm_cfg ? choose_splits(q, k, heur_blocks(q, pl.tiles_n, 64)) : 1;
  }
  pl.rowhalo = q.rowhalo;
  if (halo2_kernels) {
    // row-halo conv on 256-row tiles (one 8-wave block per CU): same K slices, half the m-tiles
    const int knob = rowhalo_knob(k, false);
    const int Wg = q.up == 2 ? q.W : q.Wo;  // (sub-pixel form: source-grid geometry, tiles must not straddle a parity)
    // (batch-invariant mode: whole tiles per SAMPLE, so that the form does not come and go with the parity of the sample count)
    if (knob == 2 && cfg == 1 && halo_runs(q, knob, L.splits) && (inv ? q.hrps % 256 == 0 : q.M % 256 == 0) &&
        (q.halo_lin || (Wg <= 256 ? 256 % Wg == 0 : Wg % 256 == 0)) && (q.up != 2 || (q.H * q.W) % 256 == 0)) {
      // one block per CU: only when the grid fills its rounds of 256 blocks (a 288-block grid would run a second round 1/8 full)
      const long blocks2 = heur_blocks(q, pl.tiles_n, 256) * L.splits;
      const long rounds = (blocks2 + 255) / 256;
      if (blocks2 * 100 >= rounds * 256 * 85) {
        pl.rowhalo = 2;
        pl.tiles_m = q.M / 256;
      }
    }
    // the staggered-wave kernel (conv_pp.hip) for the 256-row configuration, where its buffer descriptors can address the operands
    if (pl.rowhalo == 2 && q.up != 2 && q.w_bytes) {
      const bool fits = q.a_bytes && (q.C2 == 0 || q.x2_bytes) && (long)q.M / (q.Ho * q.Wo) * q.H * q.W < (1 << 24);  // the only clause that reads the sample count
      if (fits) pl.ring = 1;
      else if (inv) return fail(pl, -22, "conv2d: batch-invariant mode routes this conv to the staggered 256-pixel-tile kernel, whose buffer descriptors cannot address %d samples of %d x %d: split the call", q.M / (q.Ho * q.Wo), q.H, q.W);
    }
  }
  if (L.splits > 1) pl.scratch_bytes = (size_t)q.batch * L.splits * q.M * q.N * sizeof(float);
  choose_xcd_partition(q, L.splits, pl);
  L.tile_count = pl.tiles_n * pl.tiles_m;
  if (glds) {
    // Tail split: with two blocks per CU a grid runs in rounds of 512 blocks; T = 512 k + r with a small r costs a whole extra
    // round for r blocks (768x768 latents: 576 tiles -> the second round is 1/8 full and the conv runs at 56 % of its rate).
    // The first 512 k tiles go out as they are; the last r tiles - whole rows of m-tiles - are cut along K so that they
    // fill the chip once more for a fraction of a round, and are summed by the split-K reduce over just their rows.
    const int T = L.tile_count, nk = (q.K + BK - 1) / BK;
    const int r = T % 512, T1 = T - r;
    // (not with a transposed column range: the K-split tail would have to emit V^T from the reduce pass)
    // (off under the batch-invariant mode: which rows fall into the tail depends on the sample's position in the call)
    if (!inv && cfg == 1 && pl.rowhalo != 2 && L.splits == 1 && q.batch == 1 && T1 >= 512 && r > 0 && r <= 224 && nk >= 16 && r % pl.tiles_n == 0 &&
        q.epi != CRG_EPI_GEGLU && !(q.N & 3) && !q.vt && !q.rstat && !q.ln_stat) {
      int s2 = 512 / r;
      if (s2 > nk / 4) s2 = nk / 4;
      if (s2 > 8) s2 = 8;
      if (s2 >= 2) {
        const int row0 = (T1 / pl.tiles_n) * 128;
        pl.scratch_bytes = (size_t)s2 * (q.M - row0) * q.N * sizeof(float);
        pl.xg_s = 0;  // partial ranges use the contiguous-run order
        L.tile_count = T1;
        if (!plan_kernel(q, e, path, wnt, 1, a_f32, L, pl)) return;
        Launch& L2 = pl.tail;
        L2.tile_base = T1; L2.tile_count = r; L2.splits = s2; L2.slab_row0 = row0;
        if (!plan_kernel(q, e, path, wnt, 1, a_f32, L2, pl)) return;
        pl.route.splits = 1;  // the record describes the main launch; of the tail it keeps the kernel and the K cut
        pl.route.pair = L.pair;
        pl.route.tail_splits = s2;
        plan_reduce(q, L2, pl);
        return;
      }
    }
  }
  if (!plan_kernel(q, e, path, wnt, (glds && (cfg == 3 || cfg == 4)) ? cfg : 1, a_f32, L, pl)) return;
  if (L.splits > 1) plan_reduce(q, L, pl);
}

// which kernels take this combination of operand types and precision (the GroupNorm statistics: the bf16 path - paired epilogue / split-K
// reduce - or the fp32-class conv on pre-split planes - its fp32 epilogue)
inline void plan_problem(const Prob& q, const Env& e, Plan& pl) {
  const int a = q.a_dtype, y = q.y_dtype, prec = q.prec;
  const bool geglu = q.epi == CRG_EPI_GEGLU;
  const bool gstat_bf16 = prec == CRG_PREC_BF16 && a == CRG_BF16 && y == CRG_BF16 && (q.N & 7) == 0;
  const bool gstat_planes = (prec == CRG_PREC_BF16X3 || prec == CRG_PREC_F16MX) && a == CRG_BF16 && y == CRG_F32 && q.a_lo && !q.a_is_weight && (q.N & 3) == 0;
  if (q.gstat && !((gstat_bf16 || gstat_planes) && q.batch == 1 && q.epi == CRG_EPI_NONE))
    return fail(pl, -22, "gemm/conv: GroupNorm statistics need bf16 in / out (N %% 8 == 0) or pre-split planes in / fp32 out (N %% 4 == 0), batch 1 and a plain epilogue");
  const bool a_ok = a == CRG_BF16 || a == CRG_F32, y_ok = y == CRG_BF16 || y == CRG_F32;
  if (prec == CRG_PREC_BF16) {
    if (a_ok && y_ok) return plan_launches(q, e, P_HALF, tile_wnt(q.N, geglu), a == CRG_F32, pl);
  } else if (prec == CRG_PREC_F16MX) {
    if (q.conv && q.mx && y == CRG_F32 && q.a_lo && q.w_lo && q.epi == CRG_EPI_NONE) return plan_launches(q, e, P_PLANES, wide_wnt(q.N, false), false, pl);
  } else if (prec == CRG_PREC_BF16X3) {
    if (a == CRG_BF16 && y == CRG_F32 && q.a_lo && !q.a_is_weight && q.epi == CRG_EPI_NONE) return plan_launches(q, e, P_PLANES, tile_wnt(q.N, false), false, pl);
    if (a == CRG_F32 && y == CRG_F32) return plan_launches(q, e, P_REG_X3, tile_wnt(q.N, geglu), true, pl);
    if (!q.conv && a == CRG_BF16 && y == CRG_F32 && q.a_is_weight) return plan_launches(q, e, P_REG_X3, tile_wnt(q.N, geglu), false, pl);
  }
  fail(pl, -22, "gemm/conv: unsupported dtype/precision combination a=%d y=%d prec=%d", a, y, prec);
}

// ---- the two entry points: args (validated by crg_gemm / crg_conv2d) -> plan ----
inline Plan plan_gemm(const crg_gemm_args& a, const Env& e) {
  Plan pl;
  Prob q;
  q.M = a.M; q.N = a.N; q.K = a.K; q.batch = a.batch; q.epi = a.epilogue;
  q.a_dtype = a.a_dtype; q.y_dtype = a.y_dtype; q.prec = a.prec; q.a_is_weight = a.a_is_weight;
  q.lda = a.lda; q.ldw = a.ldw; q.ldy = a.ldy; q.y_bs = a.y_bstride; q.ldr = a.ldr; q.r_bs = a.r_bstride;
  q.bias = a.bias != nullptr; q.bias_mode = a.bias ? a.bias_mode : CRG_BIAS_NONE; q.bias_al16 = al16(a.bias);
  q.a_lo = a.a_lo != nullptr; q.w_lo = a.w_lo != nullptr;
  q.res = a.residual != nullptr; q.res_al16 = al16(a.residual); q.y_al16 = al16(a.y);
  q.gstat = a.gn_stats != nullptr; q.vt = a.vt != nullptr;
  q.rstat = a.row_stats != nullptr; q.rstat_parts = a.row_stats ? a.row_stats_parts : 0;
  q.ln_stat = a.ln_stats != nullptr; q.ln_s_al16 = !a.ln_stats || al16(a.ln_colsum);
  // what the size heuristics read: the call itself, or - batch-invariant mode - tune_samples samples of the per-sample problem
  // (a_is_weight, transposed outputs: the rows are the weight's, the samples lie along `batch`)
  const int rps = a.rows_per_sample > 0 ? a.rows_per_sample : 1;
  if (e.tune_samples > 0 && !a.a_is_weight && a.M % rps != 0) {
    fail(pl, -22, "gemm: batch-invariant mode: M=%d is not a whole number of samples of rows_per_sample=%d rows", a.M, rps);
    return pl;
  }
  set_heur(q, e, a.M, a.batch, rps, a.a_is_weight != 0);
  q.a_foot = (double)a.M * a.K * (a.a_dtype == CRG_F32 ? 4 : 2);
  q.w_foot = (double)a.N * a.K * 2;
  plan_problem(q, e, pl);
  return pl;
}

inline Plan plan_conv(const crg_conv_args& a, const Env& e) {
  Plan pl;
  Prob q;
  const int Ctot = a.C1 + a.C2;
  const bool up2 = a.upsample2x == 2;
  const int Hv = a.upsample2x ? 2 * a.H : a.H, Wv = a.upsample2x ? 2 * a.W : a.W;
  q.conv = true;
  q.M = conv_rows(a); q.N = a.Cout; q.K = conv_k(a);
  q.batch = 1; q.epi = CRG_EPI_NONE;
  q.a_dtype = a.x_dtype; q.y_dtype = a.y_dtype; q.prec = a.prec;
  q.ldw = q.K; q.ldy = q.ldr = a.Cout;
  q.bias = a.bias != nullptr; q.bias_mode = a.bias ? CRG_BIAS_COL : CRG_BIAS_NONE; q.bias_al16 = al16(a.bias);
  q.a_lo = a.x_lo != nullptr; q.w_lo = a.w_lo != nullptr;
  q.res = a.residual != nullptr; q.res_al16 = al16(a.residual); q.y_al16 = al16(a.y);
  q.cvec = a.cvec != nullptr; q.cvec_ld = conv_cvec_ld(a);
  q.gstat = a.gn_stats != nullptr; q.gstat_tile_ok = a.gn_stats != nullptr && a.gn_stats_rows != nullptr;
  q.C2 = a.C2; q.H = a.H; q.W = a.W; q.Ho = a.Ho; q.Wo = a.Wo; q.ks = a.ksize; q.up = a.upsample2x;
  q.mx = a.prec == CRG_PREC_F16MX ? 1 : 0;
  q.cm = (a.ksize == 3 && Ctot % 64 == 0) ? 1 : 0;  // must match crg_pack_weight's layout rule
  q.rowhalo = (q.cm && a.stride == 1 && a.pad_t == 1 && a.pad_l == 1 && a.Ho == Hv && a.Wo == Wv && a.C1 % 8 == 0 && a.x_dtype == CRG_BF16 &&
               ((a.y_dtype == CRG_BF16 && a.prec == CRG_PREC_BF16) ||
                (a.y_dtype == CRG_F32 && (a.prec == CRG_PREC_BF16X3 || a.prec == CRG_PREC_F16MX) && a.x_lo)))
                  ? 1 : 0;
  q.halo_lin = (a.Wo >= 16 && (a.Wo <= 128 ? 128 % a.Wo == 0 : a.Wo % 128 == 0)) ? 0 : 1;  // geometry of the output grid
  if (up2) q.halo_lin = 0;  // (geometry of the source grid: checked by crg_conv2d)
  {
    // byte sizes of x, x2 and the packed weight (buffer descriptors of conv_pp.hip); 0 = unknown / >= 2 GiB
    const double ab = (double)a.N * a.H * a.W * a.C1 * 2.0, xb = (double)a.N * a.H * a.W * a.C2 * 2.0, wb = (double)q.N * q.K * 2.0;
    const double lim = 2147483648.0;
    q.a_bytes = ab < lim ? (unsigned)ab : 0;
    q.x2_bytes = xb < lim ? (unsigned)xb : 0;
    q.w_bytes = wb < lim ? (unsigned)wb : 0;
  }
  if (a.gn_y) {
    q.gn_y = true; q.gn_gamma = a.gn_gamma != nullptr; q.gn_beta = a.gn_beta != nullptr;
    q.gn_groups = a.gn_groups; q.gn_hw = a.Ho * a.Wo;
  }
  set_heur(q, e, q.M, 1, a.Ho * a.Wo, false);  // batch-invariant mode: tune_samples samples of Ho x Wo rows
  q.a_foot = (double)a.N * a.H * a.W * Ctot * (a.x_dtype == CRG_F32 ? 4 : 2);
  q.w_foot = (double)q.N * q.K * 2 * (up2 ? 4 : 1);  // (sub-pixel form: four parity slabs)
  plan_problem(q, e, pl);
  pl.halo_lin = q.halo_lin; pl.cm = q.cm;
  pl.a_bytes = q.a_bytes; pl.x2_bytes = q.x2_bytes; pl.w_bytes = q.w_bytes;
  return pl;
}

}  // namespace crg_plan
