// crg_gemm / crg_conv2d: validation and launch of the MFMA GEMM / implicit-GEMM conv2d kernels for gfx950.
//
//   Y[m][n] = epilogue( sum_k X[m][k] * W[n][k] )      (both operands K-contiguous)
//
// No kernel lives here.  The planner (gemm_plan.h) makes every size decision; each kernel family has its own translation unit
// and exports the function that picks or launches its kernels (declared in gemm_shared.h):
//   gemm_glds_gemm.hip / gemm_glds_conv.hip (gemm_glds_kernel, gemm_glds_kernel.h), conv_rowhalo.hip (gemm_kernel of gemm_reg_kernel.h,
//   conv3_rowhalo_kernel), splitk_reduce.hip (the split-K second passes), conv_pp.hip (conv3_pp_kernel), gemm_ring.hip (gemm_ring_kernel).
#include "gemm_shared.h"
#include <cstdlib>

namespace {
using namespace crg_mm;

// ---- the launcher ------------------------------------------------------------------------------------------------------------------
// Every size decision is the planner's (gemm_plan.h): what follows fills GemmP from the plan, asks the planned family's picker for the kernel
// pointer and launches.
using crg_plan::Launch;
using crg_plan::Plan;

template <bool CONV>
KernFn pick_kernel(const Launch& L) {
  switch (L.family) {
    case crg_plan::F_GEMM_REG: return pick_reg(L, CONV);
    case crg_plan::F_GLDS: return CONV ? pick_glds_conv(L) : pick_glds_gemm(L);
    case crg_plan::F_ROWHALO: return CONV ? pick_rowhalo(L) : nullptr;
    default: return nullptr;
  }
}

template <bool CONV>
int launch_one(crg_ctx* ctx, hipStream_t st, GemmP& p, const Launch& L, double flops, double bytes) {
  p.splits = L.splits; p.ks_q = L.ks_q; p.ks_r = L.ks_r;
  p.tile_base = L.tile_base; p.tile_count = L.tile_count; p.slab_row0 = L.slab_row0;
  p.pair = L.pair;
  const bool x3 = L.family == crg_plan::F_GEMM_REG || L.ns == 2;
  const int slot = x3 ? (CONV ? CRG_K_CONV_X3 : CRG_K_GEMM_X3)
                      : (CONV ? (L.wnt == 5 ? CRG_K_CONV_W5 : L.wnt == 4 ? CRG_K_CONV_W4 : CRG_K_CONV_W1)
                              : (L.wnt == 5 ? CRG_K_GEMM_W5 : L.wnt == 4 ? CRG_K_GEMM_W4 : CRG_K_GEMM_W1));
  if (L.family == crg_plan::F_CONV_PP) {
    crg_prof_scope ps(ctx, st, slot, flops, bytes);
    return launch_conv_pp(ctx, st, p, L.wnt);
  }
  // A null pointer means that planner and switch disagree.  The planner's invariants keep it unreachable: F_GLDS with ns == 2 and every
  // F_ROWHALO with ns == 2 come from P_PLANES alone, whose y is fp32; F_ROWHALO only for convs on 128- / 160-wide tiles; F_GEMM_REG with
  // ns == 2 and a 16-bit A only for GEMMs (a_is_weight); wnt is tile_wnt / wide_wnt's 1, 4 or 5.
  const KernFn kern = pick_kernel<CONV>(L);
  if (!kern) return crg_fail(ctx, -22, "gemm/conv: no kernel for the planned launch (family %d, tile width %d)", L.family, 32 * L.wnt);
  if (int rc = crg_set_dyn_lds(ctx, reinterpret_cast<const void*>(kern), L.lds_cap, L.ns == 2 ? "gemm(planes)" : "gemm")) return rc;
  crg_prof_scope ps(ctx, st, slot, flops, bytes);
  hipLaunchKernelGGL(kern, dim3(L.grid_x, L.grid_y, 1), dim3(L.threads), L.lds, st, p);
  CRG_CHECK_LAUNCH(ctx, L.ns == 2 ? "gemm(planes)" : "gemm");
  return 0;
}

// `flops`, `bytes`: algorithmic work of the call (profiler)
template <bool CONV>
int run_plan(crg_ctx* ctx, hipStream_t st, GemmP& p, const Plan& pl, int batch, bool y_f32, double flops, double bytes) {
  if (pl.rc) return crg_fail(ctx, pl.rc, "%s", pl.msg);
  p.zero_page = (const bf16*)ctx->zero_page;
  p.tiles_n = pl.tiles_n; p.tiles_m = pl.tiles_m;
  p.xg_m = pl.xg_m; p.xg_n = pl.xg_n; p.xg_s = pl.xg_s;
  p.rowhalo = pl.rowhalo; p.ring = pl.ring; p.gstat_rows = pl.gstat_rows;
  if (pl.main.family == crg_plan::F_GEMM_RING) {
    if (int rc = launch_gemm_ring(ctx, st, p, pl.main.wnt, flops, bytes)) return rc;
    ctx->route = pl.route;
    return 0;
  }
  const bool tail = pl.tail.family != crg_plan::F_NONE;
  float* slab = nullptr;
  if (pl.scratch_bytes) {
    slab = (float*)crg_scratch(ctx, pl.scratch_bytes);
    if (!slab) return tail ? crg_fail(ctx, -12, "gemm: out of scratch for the tail slab") : crg_fail(ctx, -12, "gemm: out of scratch for %d split-K slabs", pl.main.splits);
  }
  p.slab = pl.main.splits > 1 ? slab : nullptr;
  if (tail) {
    const double T = pl.main.tile_count + pl.tail.tile_count;
    if (int rc = launch_one<CONV>(ctx, st, p, pl.main, flops * pl.main.tile_count / T, bytes * pl.main.tile_count / T)) return rc;
    p.slab = slab;
    if (int rc = launch_one<CONV>(ctx, st, p, pl.tail, flops * pl.tail.tile_count / T, bytes * pl.tail.tile_count / T)) return rc;
  } else if (int rc = launch_one<CONV>(ctx, st, p, pl.main, flops, bytes)) {
    return rc;
  }
  if (pl.reduce != CRG_REDUCE_NONE)
    if (int rc = launch_reduce(ctx, st, p, pl, batch, y_f32)) return rc;
  ctx->route = pl.route;
  return 0;
}

crg_plan::Env plan_env(const crg_ctx* ctx) { return crg_plan::Env{ctx->invariant, ctx->n_cu, dev_knobs()}; }

}  // namespace

namespace crg_mm {
// The dev knobs of the GEMM / conv dispatcher (crg_plan::Knobs), read once per process: the one place that calls getenv.
const crg_plan::Knobs& dev_knobs() {
  static const crg_plan::Knobs knobs = [] {
    crg_plan::Knobs k;
    const auto read = [](const char* name, int& v) {
      const char* s = getenv(name);
      if (s) v = atoi(s);
      return s != nullptr;
    };
    read("CRG_SPLIT_BLOCKS", k.split_blocks);
    read("CRG_SPLIT_MAX", k.split_max);
    read("CRG_GEMM_CFG", k.gemm_cfg);
    read("CRG_GEMM_D_MAX", k.d_max);
    read("CRG_GEMM_D_MAXG", k.d_max_g);
    read("CRG_CONV1_D_MAX", k.d_max_c1);
    k.rowhalo_set = read("CRG_ROWHALO", k.rowhalo);
    read("CRG_GEMM_RING", k.gemm_ring);
    read("CRG_GEMM_RING_MIN", k.gemm_ring_min);
    read("CRG_GEMM_RING_SUPER", k.gemm_ring_super);
    read("CRG_GEMM_RING_STAG", k.gemm_ring_stag);
    return k;
  }();
  return knobs;
}
}  // namespace crg_mm

extern "C" int crg_gemm(crg_ctx* ctx, void* stream, const crg_gemm_args* a) {
  if (!ctx || !a) return -22;
  ctx->route = crg_route{};
  CRG_REQUIRE(ctx, a->M > 0 && a->N > 0 && a->K > 0 && a->batch > 0, "gemm: empty problem M=%d N=%d K=%d batch=%d", a->M, a->N, a->K, a->batch);
  CRG_REQUIRE(ctx, a->K % 8 == 0, "gemm: K=%d must be a multiple of 8", a->K);
  const int ae = (a->a_dtype == CRG_F32) ? 4 : 8;  // elements per 16 B
  CRG_REQUIRE(ctx, a->lda % ae == 0 && a->ldw % 8 == 0, "gemm: lda=%ld / ldw=%ld must keep rows 16-byte aligned", (long)a->lda, (long)a->ldw);
  CRG_REQUIRE(ctx, ((uintptr_t)a->a & 15) == 0 && ((uintptr_t)a->w & 15) == 0, "gemm: operand pointers must be 16-byte aligned");
  CRG_REQUIRE(ctx, a->prec == CRG_PREC_BF16 || a->w_lo, "gemm: BF16X3 needs the lo weight plane");
  if (a->epilogue == CRG_EPI_GEGLU) {
    CRG_REQUIRE(ctx, a->N % 32 == 0, "gemm: GEGLU needs packed N %% 32 == 0 (got %d)", a->N);
    CRG_REQUIRE(ctx, !a->residual, "gemm: GEGLU epilogue takes no residual");
  }
  if (a->bias && a->bias_mode == CRG_BIAS_COL)
    CRG_REQUIRE(ctx, ((uintptr_t)a->bias & 15) == 0, "gemm: column bias must be 16-byte aligned");
  GemmP p{};
  p.a = a->a; p.a_lo = a->a_lo; p.lda = a->lda; p.a_bs = a->a_bstride;
  p.w = (const bf16*)a->w; p.w_lo = (const bf16*)a->w_lo; p.ldw = a->ldw; p.w_bs = a->w_bstride;
  p.bias = a->bias; p.bias_mode = a->bias ? a->bias_mode : CRG_BIAS_NONE;
  p.res = a->residual; p.ldr = a->ldr; p.r_bs = a->r_bstride;
  p.y = a->y; p.ldy = a->ldy; p.y_bs = a->y_bstride;
  p.M = a->M; p.N = a->N; p.K = a->K; p.epi = a->epilogue;
  p.cvec = nullptr; p.cvec_rows = 1; p.cvec_ld = 0; p.a_is_weight = a->a_is_weight;
  p.gstat = a->gn_stats; p.gstat_plane = (long)((a->M + 31) / 32) * a->N;
  p.gstat_rows = 32;
  if (a->gn_stats) CRG_REQUIRE(ctx, ((uintptr_t)a->gn_stats & 15) == 0, "gemm: gn_stats must be 16-byte aligned");
  if (a->vt) {
    const int bn_ = 32 * crg_plan::wide_wnt(a->N, false);
    CRG_REQUIRE(ctx, a->prec == CRG_PREC_BF16 && a->a_dtype == CRG_BF16 && a->y_dtype == CRG_BF16 && a->batch == 1 && a->epilogue == CRG_EPI_NONE &&
                         !a->residual && !a->gn_stats && (a->bias_mode == CRG_BIAS_COL || !a->bias),
                "gemm: a transposed column range needs a plain bf16 GEMM (no batch / residual / activation / statistics)");
    CRG_REQUIRE(ctx, a->vt_n0 > 0 && a->vt_n0 < a->N && a->vt_n0 % bn_ == 0 && a->N > 32 && a->vt_tokens > 0 && a->M % a->vt_tokens == 0 && a->vt_ld >= a->vt_tokens &&
                         ((uintptr_t)a->vt & 1) == 0,
                "gemm: transposed range n0=%d (tile %d) tokens=%d ld=%ld inconsistent with M=%d N=%d", a->vt_n0, bn_, a->vt_tokens, (long)a->vt_ld, a->M, a->N);
    p.vt = (bf16*)a->vt; p.vt_n0 = a->vt_n0; p.vt_T = a->vt_tokens; p.vt_ld = a->vt_ld;
  }
  if (a->row_stats) {
    CRG_REQUIRE(ctx, a->prec == CRG_PREC_BF16 && a->a_dtype == CRG_BF16 && a->y_dtype == CRG_BF16 && a->batch == 1 && a->epilogue == CRG_EPI_NONE &&
                         !a->gn_stats && !a->vt && !a->ln_stats && (a->N & 7) == 0 && a->row_stats_parts > 0 && a->row_stats_parts <= 64 && ((uintptr_t)a->row_stats & 15) == 0,
                "gemm: row_stats need a plain unbatched bf16 GEMM with N %% 8 == 0 (no GroupNorm statistics / transposed range / LayerNorm epilogue)");
    p.rstat = a->row_stats; p.rstat_parts = a->row_stats_parts;
  }
  if (a->ln_stats) {
    CRG_REQUIRE(ctx, a->prec == CRG_PREC_BF16 && a->a_dtype == CRG_BF16 && a->y_dtype == CRG_BF16 && a->batch == 1 && !a->residual && !a->gn_stats &&
                         (a->epilogue == CRG_EPI_NONE || a->epilogue == CRG_EPI_GEGLU) && (a->bias_mode == CRG_BIAS_COL || !a->bias) && (a->N & 3) == 0,
                "gemm: the LayerNorm epilogue needs an unbatched bf16 GEMM, N %% 4 == 0, epilogue NONE / GEGLU, no residual / row bias / statistics");
    CRG_REQUIRE(ctx, a->ln_colsum && a->ln_parts >= 2 && a->ln_parts <= 16 && (a->ln_parts & 1) == 0 && a->ln_eps >= 0.f &&
                         (((uintptr_t)a->ln_colsum | (uintptr_t)a->ln_stats) & 15) == 0,
                "gemm: ln_stats needs ln_colsum, an even number of 2..16 partials per row and 16-byte aligned pointers");
    p.ln_stat = a->ln_stats; p.ln_parts = a->ln_parts; p.ln_s = a->ln_colsum; p.ln_eps = a->ln_eps;
  }
  const double flops = 2.0 * a->M * (double)a->N * a->K * a->batch;
  const double bytes = ((double)a->M * a->K * crg_dtype_size(a->a_dtype) + (double)a->N * a->K * 2 +
                        (double)a->M * a->N * crg_dtype_size(a->y_dtype) * (a->residual ? 2 : 1)) * a->batch;
  return run_plan<false>(ctx, (hipStream_t)stream, p, crg_plan::plan_gemm(*a, plan_env(ctx)), a->batch, a->y_dtype == CRG_F32, flops, bytes);
}

extern "C" int crg_conv2d(crg_ctx* ctx, void* stream, const crg_conv_args* a) {
  if (!ctx || !a) return -22;
  ctx->route = crg_route{};
  const int Ctot = a->C1 + a->C2;
  CRG_REQUIRE(ctx, a->N > 0 && a->H > 0 && a->W > 0 && a->Cout > 0 && Ctot > 0, "conv2d: empty problem");
  CRG_REQUIRE(ctx, a->ksize == 3 || a->ksize == 1, "conv2d: ksize %d unsupported", a->ksize);
  CRG_REQUIRE(ctx, a->C1 % 8 == 0 && a->C2 % 8 == 0, "conv2d: channel counts must be multiples of 8 (C1=%d C2=%d); use crg_conv3x3_small", a->C1, a->C2);
  CRG_REQUIRE(ctx, (a->C2 == 0) == (a->x2 == nullptr), "conv2d: x2/C2 mismatch");
  CRG_REQUIRE(ctx, a->prec == CRG_PREC_BF16 || a->w_lo, "conv2d: BF16X3 / F16MX need the second weight plane");
  CRG_REQUIRE(ctx, a->Cout % 4 == 0 || !a->cvec, "conv2d: a per-sample channel vector needs Cout %% 4 == 0 (got %d)", a->Cout);
  CRG_REQUIRE(ctx, ((uintptr_t)a->x & 15) == 0 && ((uintptr_t)a->w & 15) == 0 && ((uintptr_t)a->bias & 15) == 0 && ((uintptr_t)a->cvec & 15) == 0,
              "conv2d: pointers must be 16-byte aligned");
  CRG_REQUIRE(ctx, a->upsample2x >= 0 && a->upsample2x <= 2, "conv2d: upsample2x = %d (0 none, 1 folded into the gather, 2 sub-pixel form)", a->upsample2x);
  const bool up2 = a->upsample2x == 2;
  const int Hv = a->upsample2x ? 2 * a->H : a->H, Wv = a->upsample2x ? 2 * a->W : a->W;
  if (up2) {
    // w / w_lo are the parity image of CRG_PACK_CONV_UP2; conv3_rowhalo_kernel<.., TAPS = 2> on 128-row tiles of the source grid at least
    CRG_REQUIRE(ctx, a->ksize == 3 && a->stride == 1 && a->pad_t == 1 && a->pad_l == 1 && a->Ho == Hv && a->Wo == Wv,
                "conv2d: the sub-pixel upsample form is a 3x3 / stride 1 / pad 1 conv of the upsampled image");
    CRG_REQUIRE(ctx, Ctot % 64 == 0 && a->Cout > 32, "conv2d: the sub-pixel upsample form needs Cin %% 64 == 0 and Cout > 32 (got %d, %d)", Ctot, a->Cout);
    CRG_REQUIRE(ctx, !a->x2 && !a->cvec && !a->residual && !a->gn_y, "conv2d: the sub-pixel upsample form takes no second input, channel vector, residual or fused GroupNorm");
    CRG_REQUIRE(ctx, a->x_dtype == CRG_BF16 && ((a->prec == CRG_PREC_BF16 && a->y_dtype == CRG_BF16 && !a->x_lo) ||
                                                (a->prec == CRG_PREC_BF16X3 && a->y_dtype == CRG_F32 && a->x_lo && a->w_lo)),
                "conv2d: the sub-pixel upsample form takes a 16-bit x plane: bf16 in / out, or BF16X3 on pre-split planes with fp32 output");
    CRG_REQUIRE(ctx, (a->H * a->W) % 128 == 0 && a->W >= 16 && (a->W <= 128 ? 128 % a->W == 0 : a->W % 128 == 0),
                "conv2d: the sub-pixel upsample form needs H * W %% 128 == 0 and a source width of 16..128 that divides 128, or a multiple of 128 (got %dx%d)", a->H, a->W);
  }
  CRG_REQUIRE(ctx, a->Ho > 0 && a->Wo > 0 && (a->Ho - 1) * a->stride - a->pad_t < Hv && (a->Wo - 1) * a->stride - a->pad_l < Wv,
              "conv2d: output %dx%d inconsistent with input %dx%d stride %d", a->Ho, a->Wo, Hv, Wv, a->stride);
  if (a->x_lo) {
    CRG_REQUIRE(ctx, (a->prec == CRG_PREC_BF16X3 || a->prec == CRG_PREC_F16MX) && a->x_dtype == CRG_BF16 && a->y_dtype == CRG_F32 && !a->x2 && ((uintptr_t)a->x_lo & 15) == 0,
                "conv2d: pre-split activations (x_lo) need prec BF16X3 / F16MX, 16-bit planes, fp32 output, no second input");
  }
  if (a->prec == CRG_PREC_F16MX) {
    CRG_REQUIRE(ctx, a->x_lo && a->w_lo && a->ksize == 3 && a->stride == 1 && Ctot % 64 == 0 && !a->upsample2x,
                "conv2d: F16MX takes 3x3 / stride 1 convs on MX planes (x = fp16 plane, x_lo = e4m3 pair plane, same for w / w_lo), Cin %% 64 == 0");
    for (int i = 0; i < 4; ++i) CRG_REQUIRE(ctx, a->mx_log2[i] >= -100 && a->mx_log2[i] <= 100, "conv2d: mx_log2[%d] = %d out of range", i, a->mx_log2[i]);
    CRG_REQUIRE(ctx, a->mx_log2[1] - a->mx_log2[0] == a->mx_log2[3] - a->mx_log2[2],
                "conv2d: F16MX computes both cross terms in one instruction: the lo8 / hi8 scale ratio must be the same for w (%d) and x (%d)",
                a->mx_log2[1] - a->mx_log2[0], a->mx_log2[3] - a->mx_log2[2]);
  }
  GemmP p{};
  p.a = a->x; p.a_lo = a->x_lo; p.x2 = a->x2; p.C1 = a->C1; p.C2 = a->C2; p.Ctot = Ctot;
  p.w = (const bf16*)a->w; p.w_lo = (const bf16*)a->w_lo; p.ldw = crg_plan::conv_k(*a); p.w_bs = 0;
  p.bias = a->bias; p.bias_mode = a->bias ? CRG_BIAS_COL : CRG_BIAS_NONE;
  p.res = a->residual; p.ldr = a->Cout; p.r_bs = 0;
  p.y = a->y; p.ldy = a->Cout; p.y_bs = 0;
  p.M = crg_plan::conv_rows(*a); p.N = a->Cout; p.K = crg_plan::conv_k(*a); p.epi = CRG_EPI_NONE;
  p.cvec = a->cvec; p.cvec_rows = a->Ho * a->Wo; p.cvec_ld = crg_plan::conv_cvec_ld(*a);
  p.H = a->H; p.W = a->W; p.Ho = a->Ho; p.Wo = a->Wo; p.ks = a->ksize; p.stride = a->stride;
  p.pad_t = a->pad_t; p.pad_l = a->pad_l; p.up = a->upsample2x;
  if (a->prec == CRG_PREC_F16MX) {
    // mx_log2 = {w hi8, w lo8, x hi8, x lo8}: each plane stores value * 2^s, the instruction's E8M0 scale undoes it (127 - s).
    // k-group 0 multiplies w lo8 by x hi8, k-group 1 w hi8 by x lo8.
    p.mx = 1;
    p.mx_scale[0][0] = 127 - a->mx_log2[1]; p.mx_scale[0][1] = 127 - a->mx_log2[2];
    p.mx_scale[1][0] = 127 - a->mx_log2[0]; p.mx_scale[1][1] = 127 - a->mx_log2[3];
  }
  p.gstat = a->gn_stats; p.gstat_plane = (long)((p.M + 31) / 32) * p.N;
  p.gstat_rows = 32;
  p.gstat_tile_ok = a->gn_stats != nullptr && a->gn_stats_rows != nullptr;
  if (a->gn_stats) CRG_REQUIRE(ctx, ((uintptr_t)a->gn_stats & 15) == 0 && (a->Ho * a->Wo) % 32 == 0, "conv2d: gn_stats must be 16-byte aligned and Ho * Wo a multiple of 32");
  if (a->gn_y) {
    CRG_REQUIRE(ctx, a->gn_gamma && a->gn_beta && a->gn_groups > 0 && a->Cout % a->gn_groups == 0 && a->y,
                "conv2d: the fused GroupNorm needs gamma, beta, a group count that divides Cout=%d and the raw output y", a->Cout);
    CRG_REQUIRE(ctx, (((uintptr_t)a->gn_gamma | (uintptr_t)a->gn_beta | (uintptr_t)a->gn_y) & 15) == 0, "conv2d: GroupNorm pointers must be 16-byte aligned");
    p.gn_gamma = a->gn_gamma; p.gn_beta = a->gn_beta; p.gn_eps = a->gn_eps; p.gn_groups = a->gn_groups; p.gn_silu = a->gn_silu;
    p.gn_hw = a->Ho * a->Wo; p.gn_y = a->gn_y;
  }
  const double wbytes = (double)p.N * p.K * 2 * (up2 ? 4 : 1);  // (sub-pixel form: four parity slabs; K = 4 Cin, so `flops` is the executed work)
  const double flops = 2.0 * p.M * (double)p.N * p.K;
  const double bytes = (double)a->N * a->H * a->W * Ctot * crg_dtype_size(a->x_dtype) + wbytes +
                       (double)p.M * p.N * crg_dtype_size(a->y_dtype) * (a->residual ? 2 : 1);
  const Plan pl = crg_plan::plan_conv(*a, plan_env(ctx));
  p.cm = pl.cm; p.halo_lin = pl.halo_lin;  // (K order, row-buffer form and the descriptor sizes: planner rules, plan_conv)
  p.a_bytes = pl.a_bytes; p.x2_bytes = pl.x2_bytes; p.w_bytes = pl.w_bytes;
  const int rc = run_plan<true>(ctx, (hipStream_t)stream, p, pl, 1, a->y_dtype == CRG_F32, flops, bytes);
  if (a->gn_stats_rows) *a->gn_stats_rows = pl.gstat_rows;
  if (rc || !a->gn_y || pl.gn_fused) return rc;
  // not split along K (or a shape the fused kernel does not take): the GroupNorm runs as its own launch(es) on the finished y
  return crg_groupnorm(ctx, stream, a->y, nullptr, a->Cout, a->gn_gamma, a->gn_beta, a->gn_y, a->N, a->Ho * a->Wo, a->Cout, a->gn_groups,
                       a->gn_eps, a->gn_silu, a->y_dtype);
}
