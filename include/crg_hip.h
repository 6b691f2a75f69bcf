/*
 * crg_hip.h - C-ABI of libcrg_hip.so: hand-written HIP/CDNA4 (gfx950) kernels for the
 * Stable Diffusion denoising path of HowToSD/cremage (UNet step + VAE decode/encode).
 *
 * The reference has NO native FFI: its "kernels" are PyTorch call sites inside the L6
 * compute modules.  Each entry point below replaces one family
 * of those call sites; the reference interface it replaces is cited per function
 * (paths relative to the reference root).  The Python binding a maintainer adds is
 * cremage_amd/_lib.py (ctypes); see INTEGRATION.md.
 *
 * Conventions
 *   - every pointer is a raw DEVICE pointer (tensor.data_ptr()), caller-owned;
 *   - `stream` is a hipStream_t (torch.cuda.current_stream().cuda_stream);
 *   - activations are channels-last: images [N][H][W][C] ("NHWC"), tokens [B][T][C];
 *   - all kernels are asynchronous on `stream`; no call synchronises, allocates or frees
 *     (graph-capture safe) except crg_ctx_create/destroy/reserve;
 *   - return value: 0 = ok, negative = error; text via crg_last_error(ctx).  The library
 *     never aborts (the reference's ML process has no handler, mp/mp.py:125).
 *   - one context per device, not re-entrant (the reference is single-threaded,
 *     mp/mp.py:32-127).
 */
#ifndef CRG_HIP_H
#define CRG_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 104 since the route record.  The batch-invariant mode (crg_ctx_set_invariant / crg_ctx_get_invariant and the trailing
 * crg_gemm_args.rows_per_sample) was added without a version step: two new symbols and one trailing field that is ignored while the
 * mode is off, so every caller built in this tree against 104 keeps working unchanged. */
#define CRG_VERSION 104

typedef struct crg_ctx crg_ctx;

enum crg_dtype { CRG_BF16 = 0, CRG_F32 = 1, CRG_F16 = 2 };

/* GEMM/conv arithmetic:
 *   CRG_PREC_BF16   operands rounded to bf16, one MFMA pass, fp32 accumulate;
 *   CRG_PREC_BF16X3 operands split hi+lo bf16, three MFMA passes (hi*hi + hi*lo + lo*hi),
 *                   fp32 accumulate: ~2^-17 relative operand error ("fp32-class"), used for
 *                   the VAE (pixel L-inf <= 1e-3 target) and the fp32 parity configuration. */
enum crg_prec { CRG_PREC_BF16 = 0, CRG_PREC_BF16X3 = 1,
                /* fp32-class 3x3 conv in TWO matrix passes' worth of cycles (round 4): operands as MX planes (crg_split_mx / crg_groupnorm_mx /
                 * crg_pack_weight_mx) - a fp16 plane and a plane of e4m3 pairs; main product fp16 x fp16, the two cross terms at fp8 precision
                 * on the block-scaled MX matrix instruction; fp32 accumulate and output.  Emulated pixel L-inf of the VAE decode 8e-5 (bound 1e-3) */
                CRG_PREC_F16MX = 2 };

enum crg_epilogue {
  CRG_EPI_NONE = 0,
  CRG_EPI_SILU = 1,  /* y = silu(acc + bias)                                  */
  CRG_EPI_GEGLU = 2  /* y[:, j] = (acc_v + b_v) * gelu_erf(acc_g + b_g); W packed with crg_pack_geglu */
};

enum crg_bias_mode { CRG_BIAS_NONE = 0, CRG_BIAS_COL = 1 /* bias[n] */, CRG_BIAS_ROW = 2 /* bias[m] */ };

/* ---- context ------------------------------------------------------------------------- */
int crg_version(void);
/* Which 16-bit element type this build of the library computes in: 0 = bfloat16 (libcrg_hip.so, the default and what
 * BASELINE.json configs[1] names), 1 = IEEE fp16 (libcrg_hip_f16.so: the same kernels with the _f16 matrix instructions - the
 * operand type of the reference's own GPU flow, image_generator.py:489-493,748-751).  In either build `CRG_BF16` in a dtype argument
 * means "the library's half type"; the caller must hand it tensors of that type (cremage_amd.ops does: ops.HALF).
 * Range of the fp16 build: half-type operands and results |x| <= 65504.  fp32-class operands (CRG_PREC_BF16X3) are carried as two fp16
 * planes hi = half(x), lo = half(x - hi): |x| <= 65504 as well, relative resolution 2^-22 for |x| >= 2^-3 and an absolute resolution of
 * 2^-25 below (lo is an fp16 subnormal there; conversions, LDS-DMA and the _f16 matrix instructions keep subnormals - measured, fp32-class
 * conv rel-L2 5.7e-7 against fp64, tests/test_half_type_edges.py).  With bf16 planes: fp32's range, relative resolution 2^-16. */
int crg_half_kind(void);
int crg_ctx_create(int device, crg_ctx** out);
void crg_ctx_destroy(crg_ctx* ctx);
const char* crg_last_error(crg_ctx* ctx);
/* Pre-size the context's scratch (GroupNorm partial statistics, split-K slabs). Synchronous. */
int crg_ctx_reserve(crg_ctx* ctx, size_t bytes);
/* Batch-invariant mode.  tune_samples = 0 (the state of a new context): off.  tune_samples >= 1: every decision of this library that
 * changes WHICH floating-point operations produce an output element, or their order - kernel family, tile configuration, K slices
 * and their boundaries, reduce kernel, tail split, 32- or 256-row statistics partials, GroupNorm chunking, attention kernel, LayerNorm
 * rows per wave - is taken from the PER-SAMPLE problem (rows per sample, N, K, kernel size, stride, epilogue, side channels, dtypes,
 * precision, heads, head dim) and from tune_samples alone: a size heuristic reads tune_samples * rows_per_sample where it reads the
 * call's size today.  Never from the number of samples in the call, a sample's index or what else shares the launch; the launch itself
 * (grid, XCD partition, tile order) stays that of the real size.  The result for one sample is then a function of that sample, the
 * weights and tune_samples: bit-identical alone, at any position of any batch, and on any rank of a sharded run.  The tail split is off
 * under the mode; a route whose buffer descriptors cannot address the real call is an error there, not another route.
 * Entry points with one kernel per problem class and one block per fixed tile of one sample's rows take no such decision and are
 * invariant with the mode on or off: crg_ln_gemm, crg_gemm_mx8 / crg_quant_mx8, crg_attention_x3, crg_softmax_rows, crg_conv_small.
 * Host bookkeeping only: no launch, no synchronisation.  The getter returns tune_samples (0 = off). */
int crg_ctx_set_invariant(crg_ctx* ctx, int tune_samples);
int crg_ctx_get_invariant(crg_ctx* ctx);

/* ---- per-kernel timing (bench.py roofline: HIP events on the launch stream) ------------ */
/* Between begin/end every kernel launched by a crg_* call is bracketed by hipEvents on its launch stream and
 * tagged with its kernel slot (one slot per kernel symbol as rocprofv3 prints it, see crg_kernel_name) and the
 * algorithmic FLOPs / bytes of the call.  crg_profile_end synchronises and fills `out`. */
enum crg_kernel_slot {
  CRG_K_GEMM_W1 = 0, CRG_K_GEMM_W4 = 1, CRG_K_GEMM_W5 = 2, /* gemm_glds_kernel<WNT, *, CONV=false>  bf16 LDS-DMA GEMM      */
  CRG_K_GEMM_X3 = 3,                                        /* gemm_kernel<*, *, *, *, false>        fp32 / split-bf16 GEMM */
  CRG_K_CONV_W1 = 4, CRG_K_CONV_W4 = 5, CRG_K_CONV_W5 = 6, /* conv3_pp_kernel<WNT> / conv3_rowhalo_kernel<WNT> / gemm_glds_kernel<WNT, *, CONV=true>  bf16 implicit-GEMM conv */
  CRG_K_CONV_X3 = 7,                                        /* gemm_kernel<*, *, *, *, true>         fp32-class conv (VAE)  */
  CRG_K_SPLITK = 8, CRG_K_ATTN = 9, CRG_K_GN_STATS = 10, CRG_K_GN_APPLY = 11, CRG_K_LAYERNORM = 12,
  CRG_K_ELEMENTWISE = 13, CRG_K_CONV_SMALL = 14, CRG_K_SOFTMAX = 15,
  CRG_K_LNGEMM = 16,                                        /* lngemm_kernel<WNT, KT, PAIR>          LayerNorm fused into the consuming GEMM */
  CRG_K_SLOTS = 17
};
typedef struct {
  double ms[CRG_K_SLOTS];     /* summed device time per kernel slot          */
  double flops[CRG_K_SLOTS];  /* summed algorithmic FLOPs (2*MAC)            */
  double bytes[CRG_K_SLOTS];  /* summed algorithmic (minimum) HBM bytes      */
  int64_t launches[CRG_K_SLOTS];
} crg_profile;
/* Kernel symbol (as it appears in a rocprofv3 kernel trace, template arguments abbreviated) of a slot. */
const char* crg_kernel_name(int slot);
int crg_profile_begin(crg_ctx* ctx);
int crg_profile_end(crg_ctx* ctx, void* stream, crg_profile* out);

/* ---- GroupNorm (+SiLU) ------------------------------------------------------------------
 * Replaces GroupNorm32.forward (modules/ldm/modules/diffusionmodules/util.py:214-216, eps 1e-5,
 * fp32 statistics) + nn.SiLU (openaimodel.py:207,231,754), Normalize (attention.py:189-190,
 * model.py:45-46, eps 1e-6) + `nonlinearity` (model.py:40-42).
 * x,y: [N][HW][C] of `dtype`; gamma,beta: fp32 [C].  Statistics and affine in fp32.
 * If x2 != NULL the input is the virtual channel concat [x | x2] with C = C1 + C2
 * (th.cat([h, hs.pop()], dim=1), openaimodel.py:808) and C1 % (C/groups) == 0. */
int crg_groupnorm(crg_ctx* ctx, void* stream, const void* x, const void* x2, int C1, const float* gamma,
                  const float* beta, void* y, int N, int HW, int C, int groups, float eps, int fuse_silu,
                  int dtype);
/* GroupNorm (+SiLU) of an fp32 image whose result is written as TWO bf16 planes, hi = bf16(y) and lo = bf16(y - hi) (each
 * [N][HW][C]): the operand format of the fp32-class conv (crg_conv_args.x_lo).  Same statistics and arithmetic as
 * crg_groupnorm with dtype CRG_F32; used by the VAE ResnetBlocks (model.py:128-148: norm -> swish -> conv). */
int crg_groupnorm_split(crg_ctx* ctx, void* stream, const void* x, const void* x2, int C1, const float* gamma,
                        const float* beta, void* y_hi, void* y_lo, int N, int HW, int C, int groups, float eps,
                        int fuse_silu);
/* crg_groupnorm_split for an fp32 input whose PRODUCER handed over its statistics (round 3: the fp32-class convs of the VAE emit them from
 * their epilogue like the bf16 path does, crg_conv_args.gn_stats with y_dtype = CRG_F32): `stats` = fp32 [2][N * HW / 32][C], plane 0 the
 * per 32-row block and channel sums of the conv's outputs, plane 1 of their squares.  Replaces the same `Normalize` + swish
 * (model.py:116-121 / :99-113) without the statistics pass over the fp32 tensor. */
int crg_groupnorm_pre_split(crg_ctx* ctx, void* stream, const void* x, const float* stats, const float* gamma, const float* beta,
                            void* y_hi, void* y_lo, int N, int HW, int C, int groups, float eps, int fuse_silu);
/* GroupNorm (+SiLU) whose STATISTICS come from the producer of x (and of x2): the conv / GEMM launch that wrote the tensor also wrote
 * `gn_stats` (crg_conv_args / crg_gemm_args): per 32-row block and channel the sum and the sum of squares of its rounded outputs,
 * planes [2][N * HW / 32][C1].  This call folds them per (sample, group) - one tiny launch instead of a read of the whole tensor -
 * and applies the normalisation.  Same result as crg_groupnorm up to the summation order of the statistics (fp32 partials of 32
 * values, fp64 fold).  bf16 only; HW % 32 == 0.  Reference call sites as crg_groupnorm (util.py:214-216, openaimodel.py:205-209,
 * 229-236: the GroupNorm32 + SiLU in front of each ResBlock conv).  stats2 pairs with x2 (virtual concat).  rows1 / rows2 (0 = 32): rows per
 * partial of stats1 / stats2 as their producers reported them (crg_conv_args.gn_stats_rows); with tile partials (>= 64 rows) on every
 * input the fold happens inside the normalising launch (HW / rows x C x 2 floats per sample and block) and the finalise launch is gone. */
int crg_groupnorm_pre(crg_ctx* ctx, void* stream, const void* x, const void* x2, int C1, const float* stats1,
                      const float* stats2, const float* gamma, const float* beta, void* y, int N, int HW, int C,
                      int groups, float eps, int fuse_silu, int dtype, int rows1, int rows2);
/* MX planes (CRG_PREC_F16MX, round 4) of an fp32 image [pixels][C], C % 64 == 0: x16 = fp16 [pixels][C]; x8 = [pixels][C / 64][128] bytes - per
 * 64-channel chunk 64 OCP e4m3 values of half(x) * 2^hi_log2 followed by 64 of (x - half(x)) * 2^lo_log2 (saturating).  crg_split_mx: a
 * plain tensor; crg_groupnorm_mx: GroupNorm(+SiLU) of x written in that form (`stats` = the producing conv's statistics side channel as in
 * crg_groupnorm_pre_split, or NULL for a statistics pass over x) - the VAE's Normalize + swish in front of a 3x3 conv (model.py:99-121);
 * crg_pack_weight_mx: a 3x3 conv weight [Cout][Cin][3][3] (Cin % 64 == 0) in the conv's K order, w16 [Cout][9 Cin], w8 [Cout][9 Cin / 64][128]. */
int crg_split_mx(crg_ctx* ctx, void* stream, const void* x, void* x16, void* x8, int64_t pixels, int C, int hi_log2, int lo_log2);
int crg_groupnorm_mx(crg_ctx* ctx, void* stream, const void* x, const float* stats, const float* gamma, const float* beta, void* y16, void* y8,
                     int N, int HW, int C, int groups, float eps, int fuse_silu, int hi_log2, int lo_log2);
int crg_pack_weight_mx(crg_ctx* ctx, void* stream, const void* src, int src_dtype, int n_out, int n_in, void* dst16, void* dst8, int hi_log2,
                       int lo_log2);
/* fp32 tensor -> the same two bf16 planes (n elements, n % 8 == 0): for fp32-class convs whose input does not come from a
 * GroupNorm (the VAE's Upsample / Downsample convs on the residual stream, model.py:60-64,79-86). */
int crg_split_bf16(crg_ctx* ctx, void* stream, const void* x, void* hi, void* lo, int64_t n);

/* ---- LayerNorm --------------------------------------------------------------------------
 * Replaces nn.LayerNorm(dim) in BasicTransformerBlock (attention.py:900-902,909-911).
 * x,y: [rows][dim] of `dtype`; gamma,beta fp32 [dim]. */
int crg_layernorm(crg_ctx* ctx, void* stream, const void* x, const float* gamma, const float* beta, void* y,
                  int64_t rows, int dim, float eps, int dtype);

/* ---- LayerNorm fused into the GEMM that consumes it: Y = epi(LN(X) (MxK) * W^T (NxK) + bias) --------------------
 * Replaces nn.LayerNorm + the Linear(s) behind it in BasicTransformerBlock._forward (attention.py:908-912):
 * norm1 -> to_q | to_k | to_v (:614,629,636; one launch over the row-stacked weights), norm2 -> to_q, norm3 -> the GEGLU
 * projection (:88-96).  A block keeps its 128 rows resident in LDS, normalises them in place and walks every n-tile of W:
 * X is read once and LN(X) never reaches HBM.  bf16 in / out, fp32 statistics (two-pass, as crg_layernorm).
 *   x: bf16 [M][ldx];  gamma, beta: fp32 [K];  w: bf16 [N][ldw] (crg_pack_weight; GEGLU: CRG_PACK_GEGLU);  bias: fp32 [N]
 *   (GEGLU: crg_pack_geglu_bias) or NULL;  y: bf16 [M][ldy];  epilogue: CRG_EPI_NONE | CRG_EPI_GEGLU (then y is [M][N/2]).
 * gamma == beta == NULL: no LayerNorm (plain GEMM on the same row-resident kernel, e.g. to_out + residual).
 * Built for K == 320 (the 64x64 level of SD1.5, where these GEMMs have five k-tiles and are launch / latency bound);
 * other K return an error: the caller uses crg_layernorm + crg_gemm. */
typedef struct {
  const void* x; int64_t ldx;
  const float* gamma; const float* beta; float eps;
  const void* w; int64_t ldw;
  const float* bias;
  void* y; int64_t ldy;
  int M, N, K;
  int epilogue;
  /* optional: columns n >= vt_n0 (tile aligned: multiple of 160 when N % 160 == 0, else 128) go TRANSPOSED to
   * vt[(m / vt_tokens) * (N - vt_n0) + (n - vt_n0)][m % vt_tokens] (row length vt_ld) instead of y - the V^T operand of
   * crg_attention, emitted by the same launch as Q | K.  vt == NULL: every column goes to y. */
  void* vt; int vt_n0; int vt_tokens; int64_t vt_ld;
  /* optional residual [M][ldr] (bf16) added after the bias (plain epilogue only): to_out / proj_out + skip (attention.py:685-693,1049-1057).
   * With gamma == beta == NULL the LayerNorm is skipped and the kernel is a row-resident GEMM for K = 320. */
  const void* residual; int64_t ldr;
} crg_lngemm_args;
int crg_ln_gemm(crg_ctx* ctx, void* stream, const crg_lngemm_args* args);

/* ---- GEMM: Y[b] = epi(A[b] (MxK) * W[b]^T (NxK) + bias) + residual ------------------------
 * Replaces F.linear / 1x1 nn.Conv2d call sites: to_q/to_k/to_v (attention.py:614,629,636),
 * to_out (:685), GEGLU proj + net[2] (:88-96,157-168), proj_in/proj_out (:1036,1049),
 * time_embed / emb_layers (openaimodel.py:538-543,222-228), skip_connection 1x1 (:245),
 * VAE q/k/v/proj_out/nin_shortcut (model.py:163-182,122-126), quant/post_quant_conv
 * (autoencoder.py:302-303).  Both operands are K-contiguous ("NT").
 *   a: `a_dtype` [M][lda];  w: packed by crg_pack_weight (bf16 planes) [N][ldw];
 *   bias fp32; residual/y: `y_dtype`;  cvec fp32 [M / rows_per_cvec][N] added per row group.
 * Swapping the roles of a and w yields transposed outputs (used to emit V^T for attention). */
typedef struct {
  const void* a; int64_t lda; int64_t a_bstride;
  const void* w; int64_t ldw; int64_t w_bstride;   /* hi plane                      */
  const void* w_lo;                                 /* lo plane (BF16X3) or NULL     */
  const float* bias; int bias_mode;
  const void* residual; int64_t ldr; int64_t r_bstride;
  void* y; int64_t ldy; int64_t y_bstride;
  int M, N, K, batch;
  int epilogue;
  int a_dtype, y_dtype, prec;
  int a_is_weight;   /* BF16X3 only: `a` is a packed weight (hi plane) and a_lo its lo plane */
  const void* a_lo;
  /* optional GroupNorm statistics side channel (bf16 in / out, batch 1, N % 8 == 0, plain epilogue): fp32 [2][ceil(M / 32)][N],
   * plane 0 = per 32-row block and column the sum of the rounded outputs y, plane 1 the sum of their squares (consumed by
   * crg_groupnorm_pre when y - e.g. proj_out + residual, attention.py:1049-1057 - feeds the next ResBlock's GroupNorm) */
  float* gn_stats;
  /* optional transposed column range (plain bf16 GEMM, unbatched, K below the split-K rule): output columns n >= vt_n0 - a multiple
   * of the tile width: 160 when N % 160 == 0, else 128 - go to vt[(m / vt_tokens) * (N - vt_n0) + (n - vt_n0)][m % vt_tokens] (bf16,
   * row length vt_ld >= vt_tokens) instead of y, which then has vt_n0 columns: `to_q | to_k | to_v` of a self-attention
   * (attention.py:614,629,636) as ONE launch whose V third comes out as the V^T operand of crg_attention */
  void* vt; int vt_n0; int vt_tokens; int64_t vt_ld;
  /* ---- nn.LayerNorm folded into the GEMM that consumes it, any K (attention.py:900-912: norm1 -> to_q | to_k | to_v, norm2 -> to_q,
   * norm3 -> the GEGLU projection; sgm/modules/attention.py:724-847 for SDXL) -------------------------------------------------------
   * PRODUCER side, `row_stats` (bf16 in / out, unbatched, plain epilogue, N % 8 == 0): the launch that writes the LayerNorm's input
   * (proj_in, to_out + residual, net[2] + residual) also writes, per row m, the sum and the sum of squares of its rounded outputs as
   * row_stats_parts = 2 * ceil(N / tile) column partials (tile = 160 when N % 160 == 0, else 128): fp32 [M][row_stats_parts][2]
   * (N <= 1280: at most 16 partials, which is what the consumer side takes).
   * CONSUMER side, `ln_stats` (bf16 in / out, unbatched, no residual, epilogue NONE or GEGLU, a transposed range allowed): `a` holds the
   * RAW rows x (the LayerNorm input), `w` the weight scaled by gamma and `bias` the folded bias (crg_pack_ln_weight), and
   *     y = rstd_m * (a W'^T - mean_m * ln_colsum[n]) + bias[n]  =  LayerNorm(x) W^T + b
   * with (mean_m, rstd_m) folded from the ln_parts partials per row of the producer's row_stats (fp32, eps = ln_eps, biased
   * variance as nn.LayerNorm).  The normalised tensor never exists and no LayerNorm launch runs.  K = the LayerNorm width. */
  float* row_stats; int row_stats_parts;
  const float* ln_stats; int ln_parts; const float* ln_colsum; float ln_eps;
  /* batch-invariant mode only (ignored while it is off): rows of M that belong to one sample - T for [B][T][K] tokens, H * W for a
   * 1x1 conv, M itself for a call that lies inside one sample; M must be a multiple of it.  0 means 1: the route then depends on N, K
   * and the flags only (always invariant, possibly slow).  With a_is_weight the samples lie along `batch` and the field is unused. */
  int rows_per_sample;
} crg_gemm_args;
int crg_gemm(crg_ctx* ctx, void* stream, const crg_gemm_args* args);

/* ---- conv2d as implicit GEMM ---------------------------------------------------------------
 * Replaces conv_nd(2, Cin, Cout, 3, padding=1) (openaimodel.py:208,234,551,755), stride-2
 * Downsample (:155-157), Upsample = nearest-2x + conv (:120-122; VAE model.py:60-64), the VAE
 * convs (model.py:99-113,494-498,536-540) and its asymmetric-pad stride-2 Downsample
 * (model.py:79-83, pad (0,1,0,1)).  Fused: skip concat as a second input pointer
 * (openaimodel.py:808), nearest-2x upsample in the gather, bias, per-sample channel vector
 * (the timestep-embedding add, openaimodel.py:268-277) and residual add (:279).
 *   x: [N][H][W][C1] (+ x2: [N][H][W][C2]) of `x_dtype`; w: packed [Cout][kh*kw*(C1+C2)];
 *   y/residual: [N][Ho][Wo][Cout] of `y_dtype`; cvec fp32 [N][Cout]; bias fp32 [Cout]. */
typedef struct {
  const void* x; const void* x2; int C1, C2;
  const void* w; const void* w_lo;
  const float* bias; const float* cvec;
  int64_t cvec_ld;                  /* row stride of cvec in floats (0 = Cout) */
  const void* residual;
  void* y;
  int N, H, W, Cout, Ho, Wo;
  int ksize, stride, pad_t, pad_l;  /* pad_b / pad_r are implied by Ho/Wo */
  int upsample2x;                   /* 0: none; 1: nearest-2x of x folded into the gather (any shape the conv takes); 2: the SUB-PIXEL form
                                       of the same conv - w / w_lo are the parity image (CRG_PACK_CONV_UP2) and each of the four output
                                       parities is a 2x2 conv on the source grid, 4 / 9 of the multiplies.  Needs 3x3 / stride 1 / pad 1,
                                       Ho = 2 H, Wo = 2 W, Cin % 64 == 0, Cout > 32, H * W % 128 == 0, W in {16, 32, 64, 128} or a multiple
                                       of 128, 16-bit x (prec BF16 with 16-bit y, or BF16X3 on pre-split planes), and no x2 / cvec /
                                       residual / gn_y; anything else is an error, not a fallback */
  int x_dtype, y_dtype, prec;
  const void* x_lo;                 /* BF16X3 with PRE-SPLIT activations: `x` is the bf16 hi plane, `x_lo` the bf16 lo plane
                                       (same layout; written by crg_groupnorm_split / crg_split_bf16); x_dtype = CRG_BF16,
                                       y_dtype = CRG_F32; NULL otherwise */
  float* gn_stats;                  /* optional GroupNorm statistics side channel of y (see crg_gemm_args.gn_stats; M = N * Ho * Wo rows,
                                       Ho * Wo % 32 == 0): the conv in front of a GroupNorm (openaimodel.py:208 -> :229-231, :234 -> the
                                       next block's :205-207) hands it the statistics, so the tensor is not read once more for them */
  /* optional GroupNorm(+SiLU) of the finished output - the `normalization(channels)` + `SiLU` that follows the conv inside a ResBlock
   * (openaimodel.py:208 -> :229-231; util.py:214-216): gn_y (same layout and dtype as y) = silu?(GroupNorm(y) * gn_gamma + gn_beta).
   * y is still written.  When the conv is split along K and a (sample, group) slab of the output fits one block (the 8x8 / 16x16
   * UNet levels) the launch that sums the K slices normalises as well; otherwise this is crg_conv2d followed by crg_groupnorm.
   * The result is bitwise that of the two separate calls. */
  const float* gn_gamma; const float* gn_beta; void* gn_y;
  int gn_groups; int gn_silu; float gn_eps;
  /* prec = CRG_PREC_F16MX: x / w are the fp16 planes, x_lo / w_lo the e4m3 pair planes; mx_log2 = {w hi8, w lo8, x hi8, x lo8}: the power of
   * two each fp8 half was multiplied by when it was written (crg_pack_weight_mx / crg_split_mx / crg_groupnorm_mx take the same numbers) */
  int mx_log2[4];
  /* optional OUT (host memory, written before the call returns; NULL: 32-row partials, as ever): the granularity of gn_stats this launch
   * wrote - rows per partial.  32, or the TILE height (256) where the kernel folds its waves' sums itself (round 4: the 256-pixel-tile 3x3
   * conv with the paired epilogue, Ho * Wo % 256 == 0, no K slices): plane p, partial r, channel c at gn_stats[p * plane + r * Cout + c] with
   * the SAME plane stride as the 32-row layout (ceil(M / 32) * Cout floats), only the first M / rows partials of each plane used.  Hand
   * the value to crg_groupnorm_pre (rows1 / rows2): with tile partials on every input it folds them inside the normalising launch. */
  int* gn_stats_rows;
} crg_conv_args;
int crg_conv2d(crg_ctx* ctx, void* stream, const crg_conv_args* args);

/* ---- route record: which kernel the last crg_gemm / crg_conv2d call on this context ran ---------------
 * The GEMM / conv dispatcher picks a kernel family, a tile configuration and a K cut from block counts; a test (or a profile) that wants
 * to know what a shape exercised asks here instead of restating the thresholds.  Both entry points clear the record when they are
 * entered, so after a call that failed before it launched anything `kernel` is CRG_ROUTE_NONE.  Host bookkeeping only: no launch, no
 * synchronisation.  crg_ln_gemm, crg_conv_small and crg_gemm_mx8 have one kernel each and leave the record alone. */
enum crg_route_kernel {
  CRG_ROUTE_NONE = 0,
  CRG_ROUTE_GLDS = 1,       /* gemm_glds_kernel, one plane: LDS-DMA GEMM / generic implicit-GEMM conv                                  */
  CRG_ROUTE_ROWHALO = 2,    /* conv3_rowhalo_kernel, one plane: 3x3 conv on row buffers with a halo                                    */
  CRG_ROUTE_CONV_PP = 3,    /* conv3_pp_kernel (conv_pp.hip): the staggered 256-pixel-tile 3x3 conv                                    */
  CRG_ROUTE_GEMM_RING = 4,  /* gemm_ring_kernel (gemm_ring.hip): persistent 256-row tiles                                              */
  CRG_ROUTE_GEMM_REG = 5,   /* gemm_kernel: register-staged operands (fp32 A, or fp32-class on unsplit operands)                       */
  CRG_ROUTE_PLANES = 6,     /* fp32-class / MX on pre-split planes (gemm_glds_kernel<.., NS = 2> or conv3_rowhalo_kernel, see rowhalo)      */
  CRG_ROUTE_CONVT = 7       /* conv_transpose_kernel (unblur.hip): four parity GEMMs on the source grid; wnt = tile width / 32, config = tile height / 32 */
};
enum crg_route_reduce {
  CRG_REDUCE_NONE = 0,
  CRG_REDUCE_PLAIN = 1,  /* splitk_reduce_kernel        */
  CRG_REDUCE_STATS = 2,  /* splitk_reduce_stats_kernel  (GroupNorm statistics side channel) */
  CRG_REDUCE_ROWS = 3,   /* splitk_reduce_rows_kernel   (LayerNorm row statistics)          */
  CRG_REDUCE_GN = 4      /* splitk_reduce_gn_kernel     (the GroupNorm behind the conv)     */
};
typedef struct {
  int kernel;         /* enum crg_route_kernel */
  int wnt;            /* tile width / 32: 1, 4 or 5 */
  int config;         /* tile configuration of the LDS-DMA kernel: 1 = A (128 rows, 4 waves), 3 = C (64 rows, 8 waves in two k-groups),
                         4 = D (64 rows, 4 waves); 0 where it has no meaning (ring GEMM, register-staged kernel, planes) */
  int splits;         /* K slices of the (main) launch, 1 = none */
  int tail_splits;    /* K slices of the tail launch (the last T % 512 tiles, cut along K); 0 = no tail launch */
  int rowhalo;        /* 0 = not a row-halo kernel, 1 = 128-row tiles, 2 = 256-row tiles */
  int halo_lin;       /* row-halo kernels: 1 = linear row buffer (output widths that do not tile 128) */
  int pair;           /* paired 16-bit epilogue of the main launch (LDS-DMA, row-halo and 256-pixel-tile kernels) */
  int up2;            /* sub-pixel upsample form */
  int mx;             /* CRG_PREC_F16MX */
  int reduce;         /* enum crg_route_reduce: the launch that summed the K slices */
  int gn_stats_rows;  /* rows per partial of the gn_stats side channel this call wrote (32 or 256); 0 = none asked for */
} crg_route;
int crg_last_route(crg_ctx* ctx, crg_route* out);

/* ---- weight packing -------------------------------------------------------------------------
 * src: a torch parameter as the checkpoint stores it (fp32/bf16/fp16):
 *   CRG_PACK_LINEAR   [N][K]            -> [N][K]             (nn.Linear / 1x1 conv)
 *   CRG_PACK_CONV     [Cout][Cin][k][k] -> [Cout][k*k*Cin]    K order = [tap][Cin], or, for 3x3 with Cin % 64 == 0,
 *                                                             [Cin/64][tap][64] (chunk-major: the 9 taps of one
 *                                                             64-channel slab are consecutive k-tiles -> L1 reuse)
 *   CRG_PACK_GEGLU    [2*F][K]          -> rows interleaved in 16-row groups [v0-15|g0-15|v16-31|..]
 *   CRG_PACK_CONV_UP2 [Cout][Cin][3][3] -> [4][Cout][4*Cin]   the parity image of the conv behind a nearest-2x upsample
 *                                                             (crg_conv_args.upsample2x = 2; Cin % 64 == 0): slab (a, b) holds, in
 *                                                             K order [Cin/64][u][v][64], the sums of the taps W[kh][kw] that read
 *                                                             source pixel (i + a - 1 + u, j + b - 1 + v) for output (2i + a, 2j + b):
 *                                                             kh in {0},{1,2} (a = 0) or {0,1},{2} (a = 1) for u = 0, 1; kw likewise.
 *                                                             Summed in fp32, then rounded (or split) once.  16 * Cout * Cin elements.
 *   CRG_PACK_CONVT_UP2 [Cin][Cout][4][4] -> [4][Cout][4*Cin]  the parity image of ConvTranspose2d(kernel 4, stride 2, padding 1)
 *                                                             (crg_conv_transpose2d; n_out = Cout, n_in = Cin, ksize = 4): slab (a, b)
 *                                                             holds tap W[ci][co][3 - a - 2u][3 - b - 2v], the one that reads source pixel
 *                                                             (i + a - 1 + u, j + b - 1 + v) for output (2i + a, 2j + b) - taps are
 *                                                             SELECTED, each of the 16 lands in exactly one slab, nothing is summed.
 *                                                             K order [Cin/64][u][v][64] when Cin % 64 == 0, else [u][v][Cin].
 * dst_hi (and dst_lo when non-NULL: the bf16 residual src - hi) are bf16, caller-allocated. */
enum crg_pack_kind { CRG_PACK_LINEAR = 0, CRG_PACK_CONV = 1, CRG_PACK_GEGLU = 2, CRG_PACK_CONV_UP2 = 3, CRG_PACK_CONVT_UP2 = 4 };
int crg_pack_weight(crg_ctx* ctx, void* stream, const void* src, int src_dtype, int kind, int n_out, int n_in,
                    int ksize, void* dst_hi, void* dst_lo);
/* bias for GEGLU packed the same way (fp32 in, fp32 out) */
int crg_pack_geglu_bias(crg_ctx* ctx, void* stream, const float* src, int n_out2, float* dst);
/* Operands of a GEMM that carries the LayerNorm in front of it as an epilogue correction (crg_gemm_args.ln_stats):
 *   dst_w[o][k]   = half( W[r(o)][k] * gamma[k] )                    bf16 [n_out][n_in]
 *   dst_colsum[o] = sum_k float(dst_w[o][k])                          fp32 [n_out]   (over the ROUNDED weight: what the MFMA multiplies,
 *                                                                     so that mean * colsum cancels the mean's share of the product exactly)
 *   dst_bias[o]   = sum_k W[r(o)][k] * beta[k] + bias[r(o)]           fp32 [n_out]   (bias may be NULL)
 * r(o) = o for CRG_PACK_LINEAR, the GEGLU row interleave of crg_pack_weight for CRG_PACK_GEGLU.  src: [n_out][n_in] of src_dtype.
 * Replaces the `weight` / `bias` of nn.LayerNorm (attention.py:900-902) together with the Linear behind it. */
int crg_pack_ln_weight(crg_ctx* ctx, void* stream, const void* src, int src_dtype, const float* gamma, const float* beta,
                       const float* bias, int kind, int n_out, int n_in, void* dst_w, float* dst_colsum, float* dst_bias);

/* ---- attention: O = softmax(Q K^T * scale) V ---------------------------------------------------
 * Replaces the attention core of CrossAttentionOriginal.forward (attention.py:644-658), the sliced
 * CUDA variant (:415-424) and xformers (:811): heads split 'b n (h d) -> (b h) n d', softmax over
 * keys, merge.  Flash-style (never materialises Nq x Nk).  bf16 in/out, fp32 softmax/accumulate.
 *   q: [B][Nq][ldq] (head h at column h*Dh), k: [B][Nk][ldk], vt: [B][H*Dh][ldvt] (V transposed:
 *   row = channel, column = key), o: [B][Nq][ldo].  Dh % 8 == 0, Dh <= 160. */
int crg_attention(crg_ctx* ctx, void* stream, const void* q, int64_t ldq, const void* k, int64_t ldk,
                  const void* vt, int64_t ldvt, void* o, int64_t ldo, int B, int H, int Nq, int Nk, int Dh,
                  float scale, int dtype);
/* Same attention with V ROW-MAJOR: v: [B][Nk][ldv] (head h at column h*Dh) - the layout of a fused Q|K|V (or K|V) projection
 * output, so that `to_q / to_k / to_v` of a self-attention (attention.py:614,629,636) are ONE GEMM launch over stacked
 * weights and q, k, v are column slices of its output (ldq = ldk = ldv = 3*H*Dh).  The kernel transposes V on the LDS read. */
int crg_attention_v(crg_ctx* ctx, void* stream, const void* q, int64_t ldq, const void* k, int64_t ldk,
                    const void* v, int64_t ldv, void* o, int64_t ldo, int B, int H, int Nq, int Nk, int Dh,
                    float scale, int dtype);

/* ---- row softmax (VAE AttnBlock, model.py:197-199: softmax(w * c^-0.5, dim=2)) ----------------
 * x,y: [rows][cols] of `dtype` (in place allowed), y = softmax(x * scale) per row. */
int crg_softmax_rows(crg_ctx* ctx, void* stream, const void* x, void* y, int64_t rows, int cols, int64_t ld,
                     float scale, int dtype);

/* ---- small-channel direct conv ----------------------------------------------------------------
 * conv_in (4->320, openaimodel.py:551; VAE 4->512 model.py:494; encoder 3->128 :390), conv_out
 * (320->4, :755; VAE 128->3 :536; encoder 512->8 :435) and the 1x1 quant_conv / post_quant_conv
 * (autoencoder.py:302-303): Cin <= 8 or Cout <= 8, ksize 3 (pad 1) or 1, stride 1.  Cin = 9 (the inpainting UNet's conv_in: 4 latent +
 * 1 mask + 4 masked-image channels, inpainting.yaml) takes the thin-input path too, with Cout a multiple of 8.
 * x: [N][H][W][Cin] x_dtype, w: fp32 [Cout][Cin][k][k] (checkpoint layout), bias fp32, y y_dtype. */
int crg_conv_small(crg_ctx* ctx, void* stream, const void* x, const float* w, const float* bias, void* y,
                   int N, int H, int W, int Cin, int Cout, int ksize, int x_dtype, int y_dtype);

/* ---- elementwise / layout ------------------------------------------------------------------------ */
/* timestep_embedding (util.py:151-171): out[b] = [cos(t_b f_i) | sin(t_b f_i)], f_i = exp(-ln(1e4) i/half) */
int crg_timestep_embedding(crg_ctx* ctx, void* stream, const float* t, void* out, int B, int dim, int dtype);
/* y = silu(x) (nn.SiLU in emb_layers / time_embed, openaimodel.py:222-228,538-543) */
int crg_silu(crg_ctx* ctx, void* stream, const void* x, void* y, int64_t n, int dtype);
/* NCHW (src_dtype) -> NHWC (dst_dtype) and back; used once at the UNet/VAE boundary */
int crg_nchw_to_nhwc(crg_ctx* ctx, void* stream, const void* src, void* dst, int N, int C, int HW, int src_dtype,
                     int dst_dtype);
int crg_nhwc_to_nchw(crg_ctx* ctx, void* stream, const void* src, void* dst, int N, int C, int HW, int src_dtype,
                     int dst_dtype);
/* cat([a, b], dim 1) of two NCHW tensors of src_dtype -> one NHWC tensor of dst_dtype with Ca + Cb channels, the concat folded into the
 * transpose (the hybrid conditioning's torch.cat([x] + c_concat, dim=1), ddpm.py:1520-1523, at the UNet boundary).
 * a: [N][Ca][HW], b: [N][Cb][HW], dst: [N][HW][Ca + Cb]. */
int crg_nchw2_to_nhwc(crg_ctx* ctx, void* stream, const void* src_a, const void* src_b, void* dst, int N, int Ca, int Cb, int HW,
                      int src_dtype, int dst_dtype);
/* y = a*x + b elementwise with dtype conversion (latent scaling z/0.18215, clamp((x+1)/2,0,1)) */
int crg_affine_cast(crg_ctx* ctx, void* stream, const void* x, void* y, int64_t n, float a, float b, float lo,
                    float hi, int src_dtype, int dst_dtype);

/* One k-diffusion Euler / Euler-ancestral step of an eps-prediction model under classifier-free guidance, fp32, in place on x
 * (the scalings, the guidance and the update that sit either side of the UNet call, as one kernel):
 *   den_u = x + eps_u * (-sigma), den_c = x + eps_c * (-sigma)      CompVisDenoiser.forward      k_diffusion/external.py:111-114
 *   den   = den_u + cfg_scale * (den_c - den_u)                      LDMWrapperForKDiffusion      ldm_wrapper_for_k_diffusion.py:99
 *   d     = (x - den) / sigma;   x += d * dt                         sample_euler(_ancestral)     k_diffusion/sampling.py:134-142,157-160
 *   x    += noise * noise_scale   (noise may be NULL)                ancestral noise              sampling.py:161-162
 * eps: [2][n] fp32 (unconditional half first - the batch-doubled UNet output), x / noise: [n] fp32. */
int crg_cfg_euler_step(crg_ctx* ctx, void* stream, void* x, const void* eps, const void* noise, int64_t n, float sigma,
                       float dt, float cfg_scale, float noise_scale);

/* One DDIM step with classifier-free guidance, in place on x (ddim.py:540-612 p_sample_ddim, one fp32 rounding per operation):
 *   e  = eu + cfg_scale * (ec - eu)                                   guidance
 *   x0 = (x - sqrt_one_minus_a * e) / sqrt_a                          pred_x0
 *   x  = sqrt_a_prev * x0 + dir_coef * e [+ sigma * noise]            dir_xt, noise_like
 * with the per-step scalars rounded to fp32 by the caller: sqrt_one_minus_a = sqrt(1 - a_t), sqrt_a = sqrt(a_t),
 * sqrt_a_prev = sqrt(a_prev), dir_coef = sqrt(1 - a_prev - sigma^2).  sigma == 0 reads no noise (noise may be NULL).
 * eps: [2][n] fp32 (unconditional half first), x / noise: [n] fp32. */
int crg_cfg_ddim_step(crg_ctx* ctx, void* stream, void* x, const void* eps, const void* noise, int64_t n, float cfg_scale,
                      float sqrt_one_minus_a, float sqrt_a, float sqrt_a_prev, float dir_coef, float sigma);

/* One SDXL DPM++ 2M step with classifier-free guidance, in place on x (sgm DiscreteDenoiser with EpsScaling, VanillaCFG and
 * DPMPP2MSampler.sampler_step, sampling.py:459-549; one fp32 rounding per operation, in the reference's order):
 *   den_u = eu * c_out + x,  den_c = ec * c_out + x                    c_skip = 1, c_out = -sigma (quantised)
 *   den   = den_u + cfg_scale * (den_c - den_u)                        guidance
 *   x     = m1 * x - m2 * den                                          advanced == 0 (first step, next sigma == 0)
 *   x     = m1 * x - m2 * (m3 * den - m4 * old_den)                    advanced != 0
 *   old_den = den
 * m1..m4 are the fp32 values of get_mult (sampling_utils.py / sampling.py:459-486) for the step.  old_den is read only when
 * advanced != 0 and always overwritten.  eps: [2][n] fp32 (unconditional half first), x / old_den: [n] fp32. */
int crg_cfg_dpmpp2m_step(crg_ctx* ctx, void* stream, void* x, const void* eps, void* old_den, int64_t n, float c_out, float cfg_scale,
                         float m1, float m2, float m3, float m4, int advanced);

/* One fused evaluation step of the remaining SDXL k-samplers with classifier-free guidance (sgm sampling.py:147-456 HeunEDMSampler,
 * EulerAncestralSampler, DPMPP2SAncestralSampler, :271-306 LinearMultistepSampler), in place, fp32, one rounding per operation in the
 * reference's order.  Every kind first forms the guided denoised value of the evaluation's input xin (x, or x2 for the second call of
 * a two-call step) from the raw network output eps ([2][n], unconditional half first):
 *   den_h = eps_h * c_out + xin,   den = den_u + cfg_scale * (den_c - den_u)      DiscreteDenoiser (c_skip = 1), VanillaCFG
 * then, with z = noise (read only when add_noise):
 *   EULER_A     d = (x - den) / sigma;  x = x + dt * d  [+ (z * s_noise) * sigma_up]              dt = sigma_down - sigma
 *   HEUN_1      d = (x - den) / sigma;  x2 = x + dt * d; writes x2 and d (one_call: x = x2)        sigma = sigma_hat, dt = next - sigma_hat
 *   HEUN_2      d2 = (x2 - den) / sigma;  x = x + ((d + d2) / 2) * dt                               sigma = next sigma
 *   DPMPP2S_1   x2 = m[0] * x - m[1] * den  (one_call: EULER_A's update and noise instead)
 *   DPMPP2S_2   x = m[2] * x - m[3] * den  [+ (z * s_noise) * sigma_up]
 *   LMS         d = (x - den) / sigma, written to d;  acc = coef[0] * d, acc = acc + coef[k] * hist[k - 1][i] (k < 1 + n_hist,
 *               newest first);  x = x + acc
 * A buffer a kind does not use on the step is not read (hist past n_hist, noise without add_noise, x2 / d on a one-call step). */
enum { CRG_STEP_EULER_A = 0, CRG_STEP_HEUN_1 = 1, CRG_STEP_HEUN_2 = 2, CRG_STEP_DPMPP2S_1 = 3, CRG_STEP_DPMPP2S_2 = 4, CRG_STEP_LMS = 5 };
typedef struct {
  int kind;                /* CRG_STEP_* */
  int64_t n;               /* elements of x */
  float* x;                /* [n] the sampler state, in / out */
  const float* eps;        /* [2][n] the network output of this evaluation */
  float* x2;               /* [n] HEUN_1 / DPMPP2S_1: out (the second call's input); HEUN_2 / DPMPP2S_2: in (xin) */
  float* d;                /* [n] HEUN_1: out, HEUN_2: in; LMS: this step's derivative, out */
  const float* hist[3];    /* LMS: the previous derivatives, newest first; hist[k] read only for k < n_hist */
  const float* noise;      /* [n] z, read only when add_noise */
  float c_out;             /* -sigma_q: the evaluation sigma snapped to the denoiser's table */
  float cfg_scale;
  float sigma;             /* the divisor of the kind's derivative (> 0 where one is formed) */
  float dt;
  float sigma_up, s_noise;
  float m[4];              /* DPMPP2S_1 / DPMPP2S_2 multipliers (get_mult) */
  float coef[4];           /* LMS coefficients, newest derivative first */
  int n_hist;              /* LMS: 0..3 */
  int one_call;            /* HEUN_1 / DPMPP2S_1: the step makes no second network call */
  int add_noise;           /* EULER_A, DPMPP2S_1 (one_call), DPMPP2S_2: add (z * s_noise) * sigma_up (next sigma > 0) */
} crg_sampler_step_args;
int crg_cfg_sampler_step(crg_ctx* ctx, void* stream, const crg_sampler_step_args* args);

/* One fused evaluation step of the SD1.5 k-diffusion samplers the kinds above do not cover (k_diffusion sampling.py:195-252 DPM2 and
 * DPM2 ancestral, :550-589 DPM++ SDE, :618-660 DPM++ 2M SDE, :663-710 DPM++ 3M SDE) with classifier-free guidance, in place, fp32, one
 * rounding per operation in the reference's order.  Every kind first forms the guided denoised value of the evaluation's input xin (x,
 * or x2 for DPM2_2) from the raw network output eps ([2][n], unconditional half first), as the kinds above do:
 *   den_h = eps_h * c_out + xin,   den = den_u + cfg_scale * (den_c - den_u)      CompVisDenoiser (c_out = -sigma), CFG on denoised
 * then, with z = noise (read only when add_noise):
 *   DPM2_2   d2 = (x2 - den) / sigma;  x = x + d2 * dt  [+ (z * s_noise) * sigma_up]        sigma = sigma_mid, dt = target - sigma_i
 *   SDE_1    x2 = m0 * x - m1 * den;  x2 = x2 + (z * s_noise) * sigma_up  (add_noise)       x is not written
 *   SDE_2M   den_out = den;  last: x = den;  otherwise x = a * x + c1 * den,  have_old: x = x + c2 * (den - old[0]),
 *            add_noise: x = x + ((z * p0) * p1) * s_noise
 *   SDE_3M   den_out = den;  last: x = den;  otherwise x = a * x + c1 * den,
 *            order 2: x = x + phi2 * ((den - old[0]) / r0)
 *            order 3: d10 = (den - old[0]) / r0, d11 = (old[0] - old[1]) / r1, d1 = d10 + ((d10 - d11) * r0) / rsum,
 *                     d2 = (d10 - d11) / rsum, x = (x + phi2 * d1) - phi3 * d2                      rsum = r0 + r1 in fp32
 *            add_noise: as SDE_2M
 * den_out may be a buffer the step does not read (the oldest of the history ring); it must not alias one it reads.  A buffer a kind
 * or branch does not use is not dereferenced (old[] past what the order reads or on a last step, noise without add_noise, x2 and
 * den_out of the kinds that have none). */
enum { CRG_KSTEP_DPM2_2 = 0, CRG_KSTEP_SDE_1 = 1, CRG_KSTEP_SDE_2M = 2, CRG_KSTEP_SDE_3M = 3 };
typedef struct {
  int kind;                /* CRG_KSTEP_* */
  int64_t n;               /* elements of x */
  float* x;                /* [n] the sampler state: in / out (SDE_1: in) */
  const float* eps;        /* [2][n] the network output of this evaluation */
  float* x2;               /* [n] DPM2_2: in (xin); SDE_1: out (the second call's input) */
  float* den_out;          /* [n] SDE_2M / SDE_3M: receives this step's denoised value */
  const float* old[2];     /* SDE_2M: old[0] the previous denoised value (have_old); SDE_3M: old[0], old[1] the last two (order) */
  const float* noise;      /* [n] z, read only when add_noise */
  float c_out;             /* -sigma of the evaluation */
  float cfg_scale;
  float sigma;             /* DPM2_2: the divisor sigma_mid (> 0) */
  float dt;                /* DPM2_2 */
  float sigma_up, s_noise;
  float m[2];              /* SDE_1: m0, m1 */
  float a, c1, c2;         /* SDE_2M / SDE_3M: the exponential integrator's scalars; c2: SDE_2M's midpoint correction */
  float p[2];              /* SDE_2M / SDE_3M noise: p0 = next sigma, p1 = sqrt(-expm1(-2 * eta * h)) */
  float r[2], rsum;        /* SDE_3M: r0, r1 and r0 + r1 */
  float phi2, phi3;        /* SDE_3M */
  int order;               /* SDE_3M: 1..3 */
  int last;                /* SDE_2M / SDE_3M: the next sigma is 0, x = den */
  int have_old;            /* SDE_2M */
  int add_noise;
} crg_kstep_args;
int crg_cfg_kstep(crg_ctx* ctx, void* stream, const crg_kstep_args* args);

/* Hires-fix "upscale the latents and forward-diffuse them" as one launch, fp32 NCHW, x [planes][h][w] -> out [planes][H][W]:
 *   up  = bilinear(x), align_corners = False        F.interpolate(scale_factor), image_generator.py:894,975; sdxl_image_generator.py:198
 *   out = (a * up [+ s * noise]) / d                one fp32 rounding per operation, in this order, no contraction
 * noise [planes][H][W] may be NULL (no noise term); x and noise are only read.  DDIM and k-diffusion stochastic_encode: a = sqrt(acp_t),
 * s = sqrt(1 - acp_t), d = 1; SDXL do_img2img: a = 1, s = sigma_0, d = sqrt(1 + sigma_0^2).
 * The source rows and their weights are host-built DEVICE tables, ATen's arithmetic in fp32: y_idx int32 [2][H] (row i0, then row i1 of
 * every output row), y_wt fp32 [2][H] (w0, then w1); x_idx / x_wt the same for the W columns.  up = w0y * (w0x * x[i0y][i0x] + w1x *
 * x[i0y][i1x]) + w1y * (the same on row i1y).  Indices are clamped to the source plane. */
int crg_resize_noise(crg_ctx* ctx, void* stream, const void* x, const void* noise, void* out, int64_t planes, int h, int w, int H, int W,
                     const int* y_idx, const float* y_wt, const int* x_idx, const float* x_wt, float a, float s, float d);

/* PIL's 8-bit two-pass resize (Resample.c, ImagingResampleHorizontal_8bpc / Vertical_8bpc) of a window of an image, on the device:
 * the pixel-space Lanczos glue of hires fix (ml_utils.py:28-71) and of the auto face fix (face_detector_engine.py:152-288: crop ->
 * resize -> white padding, and un-pad -> resize -> paste).  Per image n and channel c, with 32-bit integer accumulation:
 *   q      = the source, uint8, or fp32 as (uint8)(255.0f * min(max(s, 0), 1)) (truncation); rows / columns are those of the WINDOW
 *            (x0, y0, w, h): a crop, then a resize - taps never reach outside the window
 *   t[y][X] = clip8((2^21 + sum_j q[y][xmin + j] * kx[X][j]) >> 22),   (xmin, count) = x_bounds[X]     uint8 between the passes, as PIL
 *   v[Y][X] = clip8((2^21 + sum_j t[ymin + j][X] * ky[Y][j]) >> 22),   (ymin, count) = y_bounds[Y]
 *   dst[n][c][oy + Y][ox + X] = v (uint8), or out_a * ((float)v / 255.0f) + out_b (fp32: correctly rounded division, one rounding per
 *            operation, no contraction)
 * kx int32 [W][ksize_x] and x_bounds int32 [W][2], ky [H][ksize_y] and y_bounds [H][2] are host-built DEVICE tables (PIL's
 * precompute_coeffs + normalize_coeffs_8bpc).  PIL skips a pass whose input and output lengths are equal; the one-tap table
 * {2^22}, bounds (i, 1), is that skip to the bit.  Bounds are clamped to the window and to ksize, so a wrong table gives wrong
 * values, never an out-of-bounds access; they must not decrease along the axis (PIL's do not).
 * Source and destination are strided [N][C][rows][columns] tensors (strides in ELEMENTS: contiguous NCHW and channels-last alike) that
 * must not overlap.  fill != 0: every destination pixel outside the W x H rectangle at (ox, oy) is set to fill_value (a byte value
 * for an uint8 destination) by a second launch - the white square of crop_and_pad; fill == 0: nothing outside the rectangle is
 * written - the paste.  No host synchronisation, no atomics, no allocation; the intermediate t lives in LDS. */
typedef struct {
  const void* src;         /* [N][C][src_h][src_w], strided */
  int src_u8;              /* 1: uint8, 0: fp32 in [0, 1] */
  int64_t src_sn, src_sc, src_sy, src_sx; /* element strides */
  int src_h, src_w;        /* the whole source image: the window must lie inside */
  int x0, y0, w, h;        /* the window */
  int N, C;
  int W, H;                /* the result */
  const int* kx;           /* [W][ksize_x] */
  const int* x_bounds;     /* [W][2]: xmin, count */
  int ksize_x;
  const int* ky;           /* [H][ksize_y] */
  const int* y_bounds;     /* [H][2]: ymin, count */
  int ksize_y;
  void* dst;               /* [N][C][dst_h][dst_w], strided */
  int dst_u8;              /* 1: uint8, 0: fp32 */
  int64_t dst_sn, dst_sc, dst_sy, dst_sx; /* element strides */
  int dst_h, dst_w;        /* the whole destination image: the rectangle must lie inside */
  int ox, oy;              /* where the result goes */
  float out_a, out_b;      /* fp32 destination only */
  int fill;                /* != 0: write fill_value outside the rectangle */
  float fill_value;
} crg_resample_args;
int crg_resample_u8(crg_ctx* ctx, void* stream, const crg_resample_args* args);

/* Gradient-domain (Poisson) paste of a rectangle, IN PLACE on the device: OpenCV's seamlessClone NORMAL_CLONE as the reference calls
 * it with an all-white mask (face_detector_engine.py:271-286), restated from the published algorithm and NOT pinned against cv2
 * (cremage_amd.postprocess.poisson_clone_host is the definition and the fp64 yardstick).  Per image and channel, as real numbers:
 *   region  d = image[y+1 .. y+h-2][x+1 .. x+w-2], s = patch[1 .. h-2][1 .. w-2]   (hp x wp = (h-2) x (w-2): the rectangle inset by 1)
 *   mask    k[r][c] = 1 for margin <= r < hp - margin and margin <= c < wp - margin, else 0   (three 3x3 erosions: margin 3)
 *   field   vx = k ? s[r][c+1] - s[r][c] : d[r][c+1] - d[r][c],  vy the same down the rows     (forward differences)
 *   L[r][c] = vx[r][c] - vx[r][c-1] + vy[r][c] - vy[r-1][c]                                    for 1 <= r <= hp-2, 1 <= c <= wp-2
 *   solve   u[r-1][c] + u[r+1][c] + u[r][c-1] + u[r][c+1] - 4 u[r][c] = L[r][c], u = d on the region's outer ring
 *   store   image[y+2 .. y+h-3][x+2 .. x+w-3] = clip(rint(u), 0, 255), rint = half to even; nothing else is written
 * Solved directly with the type-I sine transform on the n x m = (h-4) x (w-4) interior: F = L with the ring moved to the right-hand
 * side, u = S_n ((S_n F S_m) * rden) S_m, S_k[a][b] = sin(pi (a+1)(b+1) / (k+1)), rden[a][b] = 4 / ((n+1)(m+1) (lam_n[a] + lam_m[b])),
 * lam_k[a] = 2 cos(pi (a+1) / (k+1)) - 2.  Launches: one right-hand-side kernel (integer arithmetic, exact fp32 F) and four batched
 * fp32 matrix products on v_mfma_f32_32x32x2_f32 (plain store; * rden; plain store; round / clip / uint8 store through the image's
 * strides, and the fp32 field when `field` is not NULL).  M, N and K are ragged and guarded; nothing is padded in memory.
 * image and patch are strided uint8 [N][3][rows][columns] tensors (strides in ELEMENTS = bytes: contiguous NCHW and channels-last
 * alike) that must not overlap; the patch tensor is h x w.  s_rows = S_n [n][n], s_cols = S_m [m][m], rden [n][m]: host-built fp32
 * DEVICE tables.  work: 2 * N * 3 * n * m floats.  field: contiguous fp32 [N][3][n][m] or NULL.  h >= 5 and w >= 5.
 * No atomics, no host synchronisation, no allocation; two identical calls give identical bits. */
typedef struct {
  void* image;             /* [N][3][img_h][img_w] uint8, strided, written in place */
  int64_t img_sn, img_sc, img_sy, img_sx;
  int img_h, img_w;
  const void* patch;       /* [N][3][h][w] uint8, strided */
  int64_t pat_sn, pat_sc, pat_sy, pat_sx;
  int N;
  int h, w;                /* the patch */
  int x, y;                /* its top-left corner in the image */
  int margin;
  const float* s_rows;     /* S_(h-4) */
  const float* s_cols;     /* S_(w-4) */
  const float* rden;       /* [h-4][w-4] */
  float* work;             /* 2 * N * 3 * (h-4) * (w-4) floats */
  float* field;            /* [N][3][h-4][w-4] or NULL */
} crg_poisson_args;
int crg_poisson_clone(crg_ctx* ctx, void* stream, const crg_poisson_args* args);

/* The blurred-mask composite of inpainting and spot inpainting (inpaint.py:373-392, spot_inpainter.py:1021-1039), on the device, one
 * launch: cremage_amd.postprocess.blend_blurred_mask is the definition, and the bytes are equal.  Per image:
 *   g[y][x]  = the mask's grey level: byte 0 of the mask pixel (gray_mode 0), or cv2's 14-bit fixed-point RGB -> GRAY of bytes 0..2,
 *              (r * 4899 + g * 9617 + b * 1868 + 8192) >> 14 (gray_mode 1)
 *   h[y][x]  = sum_i taps[i] * g[y][refl(x + i - 5)], v[y][x] = sum_i taps[i] * h[refl(y + i - 5)][x]   in float64: every product rounded,
 *              the sum accumulated from i = 0 upwards, NO fused multiply-add; refl = BORDER_REFLECT_101 (-1 -> 1, n -> n - 2)
 *   b        = clip(floor(v + 0.5), 0, 255)                                   cv.GaussianBlur(g, (11, 11), 0) as gaussian_blur_11 restates it
 *   m = (float)b / 255.0f, t = 1.0f - m                                        fp32, the division correctly rounded
 *   out[c]   = (uint8) trunc(clip(updated[c] * m + original[c] * t, 0, 255))  fp32, one rounding per operation, channels c < C
 * taps: the eleven normalised Gaussian taps (sigma 2) as the HOST computes them - the device calls no exp.
 * original, updated and out are strided uint8 images [N][H][W][C], C in 1..4, channels adjacent (pixel stride 3 or 4 bytes for RGB
 * in an RGB or RGBA buffer); mask [N][H][W][1, 3 or 4].  Strides in bytes; mask_sn may be 0 (one mask for every image).  out may BE
 * original (same pointer and strides: in place); otherwise out must not overlap original, and never updated or the mask.
 * Window (win_w > 0): the caller states that every grey level outside the rectangle (win_x, win_y, win_w, win_h) INSET by 5 is 0, i.e.
 * the rectangle is the bounding box of the non-zero grey levels grown by 5 (clamped to the image).  Tiles that do not touch it skip the
 * blur: there m = 0 and the result is the original byte, exactly, so the bytes equal the run without a window.  win_w == 0: no window.
 * H >= 6 and W >= 6 (what a radius-5 reflect-101 accepts).  No atomics, no host synchronisation, no allocation, no scratch. */
typedef struct {
  const void* original;    /* [N][H][W][C] uint8 */
  int64_t org_sn, org_sy, org_sx;
  const void* updated;     /* [N][H][W][C] uint8 */
  int64_t upd_sn, upd_sy, upd_sx;
  const void* mask;        /* [N][H][W][1 | 3 | 4] uint8 */
  int64_t msk_sn, msk_sy, msk_sx;
  int gray_mode;           /* 0: byte 0 as is, 1: cv2 RGB -> GRAY of bytes 0..2 */
  void* out;               /* [N][H][W][C] uint8; may be `original` */
  int64_t out_sn, out_sy, out_sx;
  int N, H, W, C;
  int win_x, win_y, win_w, win_h; /* win_w == 0: the whole image */
  double taps[11];
} crg_blend_args;
int crg_blur_blend_u8(crg_ctx* ctx, void* stream, const crg_blend_args* args);

/* y = a*x + b*y elementwise (IP-Adapter FaceID: out + ipa_scale * out_ipa, attention.py:681;
 * ControlNet residual adds, cldm.py:57-65) */
int crg_axpby(crg_ctx* ctx, void* stream, const void* x, void* y, int64_t n, float a, float b, int dtype);

/* ---- MX8: block-scaled e4m3 operands for the feed-forward GEMMs (opt-in: FeedForward(precision="mx8"), CRG_FF_MX8=1) ------------------
 * An MX8 matrix of logical shape [R][K], K % 32 == 0, is two byte planes:
 *   q: uint8 [R][K]       OCP e4m3fn codes (bias 7, no infinities, largest finite 448)
 *   e: uint8 [R][K / 32]  E8M0: the 32 elements q[r][32 b .. 32 b + 31] are multiplied by s = 2^(e[r][b] - 127)
 * Scale rule per 32-element block, on the fp32 value of each element, a = the block's largest magnitude:
 *   a == 0: e = 127 and every code is 0.  Otherwise a = m 2^E with m in [1, 2): e - 127 = E - 8 when m <= 1.75, else E - 7 - the smallest
 *   power of two with a / s <= 448, so nothing clips - and e is clamped to [0, 254].  Codes are x / s rounded to nearest-even into e4m3,
 *   saturating at +-448 (reachable only where e was clamped); a value that rounds to zero has code 0 whatever its sign.  Inputs are
 *   finite.  ops.quant_mx8_host restates the rule in plain torch; the kernels are bit-exact to it.
 * crg_quant_mx8: x = [M][K] of the library's half type with row stride ldx (elements; any alignment) -> q [M][K], e [M][K / 32], dense.
 * crg_pack_weight_mx8: a Linear weight src [n_out][n_in] (fp32 / bf16 / fp16, dense) -> the planes the GEMM reads: q [n_out][n_in] and
 *   e [n_out][n_in / 32] in the row order of crg_pack_weight (CRG_PACK_LINEAR: as is; CRG_PACK_GEGLU: value / gate rows interleaved in
 *   16-row groups, n_out % 32 == 0); the rule runs along n_in.
 * crg_gemm_mx8: Y = epi(A W^T + bias) (+ residual) on v_mfma_scale_f32_16x16x128_f8f6f4, every 32-element block of either operand under
 *   its own scale, fp32 accumulation.  M >= 1 arbitrary; K % 64 == 0; N % 32 == 0 (rows of W, before the GEGLU halving).  Anything else is
 *   an error (-22): there is no fallback.  Not offered: batch, split-K, transposed ranges, GroupNorm / LayerNorm statistics.
 * Profile slots: the GEMM counts under CRG_K_GEMM_W1 (family "gemm"), the quantisers under CRG_K_ELEMENTWISE. */
enum crg_mx8_out { CRG_MX8_OUT_HALF = 0, CRG_MX8_OUT_F32 = 1, CRG_MX8_OUT_MX8 = 2 };
typedef struct {
  const void* a_q; int64_t lda;      /* uint8 [M][lda]; 16-byte aligned rows */
  const void* a_e; int64_t lde;      /* uint8 [M][lde] */
  const void* w_q; const void* w_e;  /* crg_pack_weight_mx8: [N][K], [N][K / 32] */
  const float* bias;                 /* fp32 [N] or NULL (GEGLU: crg_pack_geglu_bias) */
  const void* residual; int64_t ldr; /* half type [M][ldr] or NULL; CRG_EPI_NONE only */
  void* y; int64_t ldy;              /* y_kind HALF: half type, F32: float, MX8: uint8 codes; [M][ldy], ldy % 4 == 0, 16-byte aligned base */
  void* y_e; int64_t ldye;           /* y_kind MX8: uint8 [M][ldye] scales; the output width must be a multiple of 64 then */
  int M, N, K;
  int epilogue;                      /* CRG_EPI_NONE | CRG_EPI_GEGLU (erf form; the output is [M][N / 2]) */
  int y_kind;                        /* enum crg_mx8_out */
} crg_mx8gemm_args;
int crg_quant_mx8(crg_ctx* ctx, void* stream, const void* x, int64_t ldx, void* q, void* e, int64_t M, int K);
int crg_pack_weight_mx8(crg_ctx* ctx, void* stream, const void* src, int src_dtype, int kind, int n_out, int n_in, void* dst_q, void* dst_e);
int crg_gemm_mx8(crg_ctx* ctx, void* stream, const crg_mx8gemm_args* args);

/* ---- flash attention for the fp32 class (opt-in: ops.attention(..., flash=True), CRG_ATTN_X3=1) ------------------------------------------
 * O = softmax(Q K^T * scale) V on fp32 tensors in ONE launch for all batches, heads and query blocks.  Replaces, for fp32 inputs, the
 * host loop of the unfused route: per image and query chunk a hi / lo split of K and V^T, a batched QK^T GEMM into an fp32 score buffer,
 * the row softmax and a batched PV GEMM.  Here the hi / lo planes of Q, K, V and P are made inside the kernel (registers / LDS), there is
 * no plane tensor, no score buffer and no workspace: memory does not grow with Nq x Nk.
 *   q  fp32 [B][Nq][ldq], head h at column h*Dh      k fp32 [B][Nk][ldk]      (q and k may be column slices of one projection output)
 *   vt fp32 [B][H*Dh][ldvt]: V transposed            o fp32 [B][Nq][ldo]
 * Arithmetic of the class: S = Qh Kh + Qh Kl + Ql Kh and O += Ph Vh + Ph Vl + Pl Vh on the half-type MFMA with fp32 accumulation;
 * running max, exp, row sum and rescale in fp32.  Keys >= Nk are masked by selection and their memory is never read: rows of k past Nk
 * and columns Nk..ldvt of vt may hold anything, NaN included.  Bitwise deterministic (no atomics, no key split).
 * Domain: Dh % 8 == 0, 8 <= Dh <= 512; Nq >= 1; 1 <= Nk <= ldvt; B, H in 1..65535; ldq, ldk, ldo >= H*Dh and multiples of 4 with
 * 16-byte aligned q, k, o; vt 4-byte aligned with any ldvt (rows are read as float4 when ldvt % 4 == 0 and vt is 16-byte aligned).
 * Anything else is an error (-22): there is no fallback.  Profile slot: CRG_K_ATTN. */
typedef struct {
  const float* q; int64_t ldq;
  const float* k; int64_t ldk;
  const float* vt; int64_t ldvt;
  float* o; int64_t ldo;
  int B, H, Nq, Nk, Dh;
  float scale;
} crg_attn_x3_args;
int crg_attention_x3(crg_ctx* ctx, void* stream, const crg_attn_x3_args* args);

/* ---- temporal layers of the video UNet (video.hip) ----------------------------------------------------------------------------------------
 * Activations are [b*T*S][C] rows: video v, frame t, pixel s at row (v*T + t)*S + s - the bytes of a [(b t), h, w, C] channels-last tensor.
 *
 * crg_conv_frames: the (3, 1, 1) conv along the frame axis,
 *     y[v,t,s,:] = sum_{d=-1,0,1} W_d x[v,t+d,s,:] + bias [+ cvec[v*T+t,:]],   then, with a residual,  y = residual + rscale[v*T+t] * y
 *   (rscale NULL = 1).  Frames outside [0, T) contribute zero BY SELECTION: their rows - another video's, or outside the tensor - are never
 *   read, so a NaN there cannot reach y.  x half type [b*T*S][Cin]; w half type [Cout][3*Cin], tap-major (column d*Cin + c = weight
 *   [o][c][d][0][0]; crg_pack_weight CRG_PACK_LINEAR of that permuted matrix); bias fp32 [Cout] or NULL; cvec fp32 [b*T][cvec_ld] or NULL;
 *   residual half type [b*T*S][Cout] or NULL; rscale fp32 [b*T] or NULL (needs residual); y half type [b*T*S][Cout], may alias residual.
 *   fp32 accumulation over the whole K = 3*Cin in one block, fixed order; the tile shape depends on Cout alone: a row's bits are a function
 *   of its own video and the weights, with the batch-invariant mode on or off.
 *   Domain: Cin, Cout multiples of 32; b, T, S >= 1; b*T*S < 2^31 - 128; all pointers 16-byte aligned; cvec_ld >= Cout, a multiple of 4.
 *   Profile slot: CRG_K_CONV_W4 (128-wide tiles) / CRG_K_CONV_W1.
 *
 * crg_attention_frames: for every (video, pixel, head)  o = softmax(q k^T * scale) v  over the T frames.  q, k, v: `dtype` (CRG_BF16 = the
 *   half type, or CRG_F32) [b*T*S][ld*], head h at column h*Dh - column ranges of one fused projection output, V row-major; o `dtype`
 *   [b*T*S][ldo].  Products, softmax and sums in fp32 on the vector unit.  One kernel per (dtype, head-width class), no decision from b.
 *   Domain: 1 <= T <= 32 (more frames: -22), Dh a multiple of 8 in 8..64, b <= 65535, row strides >= H*Dh and multiples of 16 bytes,
 *   pointers 16-byte aligned.  Profile slot: CRG_K_ATTN.
 *
 * crg_add_frames:     y[r][:] = x[r][:] + e[r / S][:]             x, y `dtype` [frames*S][C], e `dtype` [frames][C]; C % 8 == 0; y may be x.
 * crg_lincomb_frames: y = a[f] * x + c[f] * z per frame f         x, z, y `dtype` [frames][per_frame] dense, a / c fp32 [frames] or NULL (= 1,
 *   product skipped); per_frame % 8 == 0.  Each product and the sum are rounded separately in fp32 (no FMA), then once to `dtype`.
 *   Profile slot of both: CRG_K_ELEMENTWISE. */
typedef struct {
  const void* x; const void* w;
  const float* bias;
  const float* cvec; int64_t cvec_ld;
  const void* residual; const float* rscale;
  void* y;
  int b, T, S, Cin, Cout;
} crg_conv_frames_args;
int crg_conv_frames(crg_ctx* ctx, void* stream, const crg_conv_frames_args* args);
typedef struct {
  const void* q; int64_t ldq;
  const void* k; int64_t ldk;
  const void* v; int64_t ldv;
  void* o; int64_t ldo;
  int b, T, S, H, Dh;
  float scale;
  int dtype;
} crg_attn_frames_args;
int crg_attention_frames(crg_ctx* ctx, void* stream, const crg_attn_frames_args* args);
int crg_add_frames(crg_ctx* ctx, void* stream, const void* x, const void* e, void* y, int64_t frames, int S, int C, int dtype);
int crg_lincomb_frames(crg_ctx* ctx, void* stream, const float* a, const void* x, const float* c, const void* z, void* y, int64_t frames,
                       int64_t per_frame, int dtype);

/* ---- temporal layers of the video VAE decoder (video_x3.hip) ---------------------------------------------------------------------------
 * Rows as above: video v, frame t, pixel s at row (v*T + t)*S + s.
 *
 * crg_conv_frames_x3: crg_conv_frames in the fp32 class - same formula, same zero padding BY SELECTION (a frame outside its video is never
 *   addressed).  x arrives as the two half-type planes x_hi, x_lo [b*T*S][Cin] that crg_groupnorm_split / crg_split_bf16 write; w as the
 *   planes w_hi, w_lo [Cout][3*Cin] of crg_pack_weight(CRG_PACK_LINEAR, split) applied to the tap-major matrix of crg_conv_frames; bias,
 *   cvec, rscale fp32 as there; residual fp32 [b*T*S][Cout] or NULL; y fp32 [b*T*S][Cout], may alias residual.  Three matrix passes
 *   lo*hi + hi*lo + hi*hi per k-step into one fp32 accumulator over the whole K = 3*Cin in one block, fixed order, no split-K; the tile
 *   shape depends on Cout alone (batch-invariant with the mode on or off).
 *   Domain: that of crg_conv_frames; y must not overlap x_hi / x_lo, nor the residual at an offset (-22).  Profile slot: CRG_K_GEMM_X3.
 *
 * crg_conv_frames_thin: the same conv on C <= 8 channels (AE3DConv.time_mix_conv, the decoder's 3 pixel channels).  x, y `dtype`
 *   (CRG_BF16 = the half type, or CRG_F32) [b*T*S][C], y must not overlap x anywhere (-22); w fp32 [C][C][3] (the Conv3d weight [C][C][3][1][1]); bias fp32
 *   [C] or NULL.  One thread per pixel: y = bias, then for tap d = -1, 0, 1 (skipped when frame t + d is outside the video: never read)
 *   and input channel ci in ascending order  y[co] = fma(w[co][ci][d], x[v,t+d,s,ci], y[co])  in fp32, rounded once to `dtype`.
 *   Profile slot: CRG_K_ELEMENTWISE. */
typedef struct {
  const void* x_hi; const void* x_lo;
  const void* w_hi; const void* w_lo;
  const float* bias;
  const float* cvec; int64_t cvec_ld;
  const void* residual; const float* rscale;
  void* y;
  int b, T, S, Cin, Cout;
} crg_conv_frames_x3_args;
int crg_conv_frames_x3(crg_ctx* ctx, void* stream, const crg_conv_frames_x3_args* args);
int crg_conv_frames_thin(crg_ctx* ctx, void* stream, const void* x, const float* w, const float* bias, void* y, int b, int T, int S, int C,
                         int dtype);

/* ---- data movements of the FILM frame interpolator (film.hip) --------------------------------------------------------------------------
 * Channels-last fp32 rows: pixel (n, y, x) of an [N, H, W] tensor is row (n*H + y)*W + x, its channels consecutive, rows `ld` ELEMENTS
 * apart.  A pointer carries its channel offset already, so a destination may be a column slice [off, off + C) of a wider buffer (the
 * reference's torch.cat as a write); a kernel never touches the other columns.  Pointers need their element's alignment only; 16-byte
 * accesses are used where pointers, strides and C allow.  Sources and destinations of one call must not overlap, except crg_film_act's
 * y == x.  Profile slot: CRG_K_ELEMENTWISE.
 *
 * crg_film_warp: backward warp (frame_interpolation_pytorch util.warp).  dst[n,y,x,c] = bilinear(src[n], x + s*flow[n,y,x,0],
 *   y + s*flow[n,y,x,1])[c], c < C: the position is clamped to [0, W-1] x [0, H-1] (grid_sample padding_mode 'border', align_corners
 *   False), s = scale[n] (fp32 [N]) or 1 for NULL.  Up to 64 lanes share a pixel; each of them reads the pixel's flow (one broadcast access)
 *   and computes the four weights once, then walks its share of the C channels - the weights are per lane, not per channel.  An integral
 *   position returns the source pixel bit for bit.  dst fp32 and / or the half-type planes hi = half(v), lo = half(v - hi), rows ld_planes apart.
 * crg_film_pool2: F.avg_pool2d(x, 2, 2): dst [N, H/2, W/2] (floor), ((a + b) + c + d) * 0.25 in reading order.
 * crg_film_flow_up: dst = residual + F.interpolate(2*v, size = (2h, 2w), mode 'bilinear') on 2 channels; v [N, h, w], residual (or NULL)
 *   and dst [N, 2h, 2w].
 * crg_film_act: y = scale[n] * (x >= 0 ? x : slope*x) of x [N, H, W] x C (scale fp32 [N], or NULL: no product; slope 1 makes it a scaled
 *   copy into a slice, which is how multiply_pyramid's dt / 1 - dt reach the fusion's input), as fp32 (y, may be x itself), as planes (hi, lo) and / or as its 2 x 2 mean
 *   (pool [N, H/2, W/2], floor) - any non-empty subset, one pass over x. */
typedef struct {
  const float* src; int64_t ld_src;
  const float* flow; int64_t ld_flow;
  const float* scale;
  float* dst; int64_t ld_dst;
  void* hi; void* lo; int64_t ld_planes;
  int N, H, W, C;
} crg_film_warp_args;
int crg_film_warp(crg_ctx* ctx, void* stream, const crg_film_warp_args* args);
int crg_film_pool2(crg_ctx* ctx, void* stream, const float* src, int64_t ld_src, float* dst, int64_t ld_dst, int N, int H, int W, int C);
int crg_film_flow_up(crg_ctx* ctx, void* stream, const float* v, int64_t ld_v, const float* residual, int64_t ld_res, float* dst, int64_t ld_dst,
                     int N, int h, int w);
typedef struct {
  const float* x; int64_t ld_x;
  float* y; int64_t ld_y;
  void* hi; void* lo; int64_t ld_planes;
  float* pool; int64_t ld_pool;
  const float* scale;
  int N, H, W, C;
  float slope;
} crg_film_act_args;
int crg_film_act(crg_ctx* ctx, void* stream, const crg_film_act_args* args);

/* ---- the face unblur / colorize network (unblur.hip; modules/unblur_face/cremage_model_v6.py) ------------------------------------------
 * crg_conv_transpose2d: nn.ConvTranspose2d(Cin, Cout, kernel 4, stride 2, padding 1) in the fp32 class, one launch for all four output
 *   parities:  y[n][2i+a][2j+b] = bias + sum_{u,v in {0,1}} W[:, :, 3-a-2u, 3-b-2v]^T x[n][i+a-1+u][j+b-1+v], x outside the image = 0 by
 *   selection (never addressed), then SiLU when `silu` (ConvTransposeAct, cremage_model_v6.py:395-396).  x_hi, x_lo: the half-type planes
 *   [N*H*W][Cin] of crg_split_bf16 / crg_groupnorm_add_act; w_hi, w_lo: crg_pack_weight(CRG_PACK_CONVT_UP2, split); bias fp32 [Cout] or
 *   NULL; y fp32 [N][2H][2W][Cout] channels-last, dense, not overlapping the planes.  No zero-stuffed image and no zero tap exists; on a
 *   grid of one row (column) the taps no pixel reaches are not read.  Three matrix passes lo*hi + hi*lo + hi*hi per k-step into one fp32
 *   accumulator, whole K in one block, fixed order.  Cin % 8 == 0, Cout % 4 == 0, any H, W >= 1; pointers 16-byte aligned.  Sets the
 *   route record (CRG_ROUTE_CONVT).  Profile slot: CRG_K_CONV_X3.
 *
 * crg_groupnorm_add_act: y = silu?(GroupNorm(x) * gamma + beta + skip) - the tail `x = gn2(x); x = x + skip; x = act2(x)` of the
 *   post-norm residual blocks (cremage_model_v6.py:94-98, :194-198), and with skip = NULL the `gn1` + `act1` in front of conv2.  x fp32
 *   [N][HW][C] dense; skip fp32 or NULL, rows ld_skip elements apart; y fp32 (or NULL) rows ld_y apart; y_hi / y_lo (both or none) the
 *   half-type planes hi = half(y), lo = half(y - hi), rows ld_planes apart - a destination may be a column slice of a wider buffer, the
 *   other columns are not touched.  gn_stats: the side channel [2][N*HW/32][C] of the conv that produced x (crg_conv_args.gn_stats), or
 *   NULL: the statistics are then summed from x.  Either way they are folded in fp64.  workspace: N * groups * 64 * 16 bytes at most.
 *   C % 8 == 0, groups <= 64 dividing C (any group size), HW >= 1.  Two launches.  Profile slots: CRG_K_GN_STATS, CRG_K_GN_APPLY. */
int crg_conv_transpose2d(crg_ctx* ctx, void* stream, const void* x_hi, const void* x_lo, const void* w_hi, const void* w_lo, const float* bias, void* y,
                         int N, int H, int W, int Cin, int Cout, int silu);
int crg_groupnorm_add_act(crg_ctx* ctx, void* stream, const void* x, const void* skip, int64_t ld_skip, const float* gamma, const float* beta,
                          const float* gn_stats, void* y, int64_t ld_y, void* y_hi, void* y_lo, int64_t ld_planes, void* workspace,
                          int64_t workspace_bytes, int N, int HW, int C, int groups, float eps, int silu);

/* ---- the glue of face unblur / colorize (warp_paste.hip; cremage_amd.postprocess.warp_affine_u8 / paste_warped_face are the definitions) ----
 * Both warp a uint8 image with a 2 x 3 destination-to-source map m = (m00, m01, m02, m10, m11, m12), six float64 values per map behind a
 * HOST pointer that is read when the call is made: the coefficients travel as kernel arguments, nothing is uploaded or cached.  Per
 * destination pixel (x, y), in IEEE double, every operation rounded on its own (no fused multiply-add), cut(v) = (int64) clip(rint(v),
 * -2^40, 2^40) with rint half to even:
 *   ax = cut(m00 * x * 1024), bx = cut(m10 * x * 1024), x0 = cut((m01 * y + m02) * 1024) + 16, y0 = cut((m11 * y + m12) * 1024) + 16
 *   X = (x0 + ax) >> 5, Y = (y0 + bx) >> 5            the source position in 1 / 32 pixel; 64-bit, arithmetic shifts (towards -inf)
 *   sx = X >> 5, fx = X & 31, sy = Y >> 5, fy = Y & 31
 *   s[c] = sum over the four neighbours (sx + dx, sy + dy) INSIDE the source of (dx ? fx : 32 - fx) * (dy ? fy : 32 - fy) * 32 * src[..][c]
 *   warped[c] = (s[c] + 2^14) >> 15                    integers throughout; a neighbour outside the source counts 0 and is never read
 * Images are strided, channels adjacent, C in 1..4: views are fine (a window of a larger image, the RGB of an RGBA buffer).
 *
 * crg_warp_affine_u8: N destination images of one source in one call (one launch per 16 maps).  src uint8 [h][w][C], strides in bytes;
 *   dst_to_src 6 * N doubles; dst_f32 = 0: dst uint8 [N][H][W][C], strides in bytes, dst_sc = 1; dst_f32 = 1: dst fp32 [N][C][H][W],
 *   strides in ELEMENTS, holding (float)warped / 255.0f with the division correctly rounded - torch's .float() / 255.0 of the bytes, in
 *   the layout the network reads.  dst must not overlap src.
 * crg_paste_warped_u8: paste_warped_face in one launch, IN PLACE on image uint8 [H][W][C] (strides in bytes).  face: uint8 [h][w][C]
 *   (face_f32 = 0, face_sc = 1) or fp32 [C][h][w] (face_f32 = 1), strides in ELEMENTS of its type; an fp32 value v is read as the byte
 *   (uint8)(fminf(fmaxf(v, 0), 1) * 255.0f) - one fp32 product, truncation: clamp(0, 1).mul(255).byte(); values are finite.  Per pixel
 *   and channel: warped as above, mask = warped > 0, eroded 5 x 5 where neighbours outside the IMAGE do not constrain, and where the
 *   eroded mask is set the warped byte is stored.  No other byte of the image is written, none is read; a pixel may take some channels
 *   and keep others.  rect (x, y, w, h), inside the image: the caller's statement that warped is 0 outside it
 *   (postprocess.warped_footprint); only the 64 x 16 tiles that touch it are launched, halo pixels are computed from the map whatever the
 *   rectangle says, so a correct rectangle changes no byte.  An empty rectangle launches nothing.  The face must not overlap the image.
 * Errors (-22, before any launch): C outside 1..4, an empty size, a pixel stride smaller than C, a negative stride, a coefficient that is
 * not finite, overlap.  No atomics, no host synchronisation, no allocation, no scratch.  Profile slot: CRG_K_ELEMENTWISE. */
int crg_warp_affine_u8(crg_ctx* ctx, void* stream, const void* src, int64_t src_sy, int64_t src_sx, int h, int w, int C, const double* dst_to_src,
                       int N, void* dst, int dst_f32, int64_t dst_sn, int64_t dst_sc, int64_t dst_sy, int64_t dst_sx, int H, int W);
int crg_paste_warped_u8(crg_ctx* ctx, void* stream, void* image, int64_t img_sy, int64_t img_sx, int H, int W, int C, const void* face,
                        int face_f32, int64_t face_sc, int64_t face_sy, int64_t face_sx, int h, int w, const double* face_from_image, int rect_x,
                        int rect_y, int rect_w, int rect_h);

/* ---- ControlNet's HED annotator (annot.hip; modules/annotator/hed/__init__.py) ----------------------------------------------------------
 * crg_relu_pool_proj: everything that follows one conv of the VGG trunk, in one pass over the conv's fp32 output x [N][H][W][C] (dense,
 *   channels-last).  r = x > 0 ? x : 0 (so -0 and NaN give +0); any non-empty subset of
 *     hi, lo            half-type planes [N][H][W][C]: hi = half(r), lo = half(r - hi), bit-equal to crg_split_bf16 of r
 *     pool_hi, pool_lo  the same planes of maxpool2x2(r), [N][H/2][W/2][C], stride 2, floor: the last row / column of an odd size is in
 *                       no window (F.max_pool2d(r, 2, 2))
 *     proj              fp32 [N][H][W]: proj_bias[0] + sum_c proj_w[c] * r[c] - the block's 1 x 1 `projection` conv; proj_w fp32 [C],
 *                       proj_bias one fp32 on the device or NULL (0).  Order:
 *                       per group of 8 consecutive channels acc = fma(w[c], r[c], acc) from 0 in channel order, then the C / 8 group
 *                       sums - C / 8 a power of two up to 64: an xor butterfly over the group index, offsets 1, 2, ..; otherwise: added
 *                       in group order - then + proj_bias.  A function of C alone: not of N, H, W, the grid or the batch-invariant mode.
 *   A pair of planes is both or none.  Every element of x is read exactly once; no atomics, no workspace, no scratch.  C % 8 == 0,
 *   8 <= C <= 2048; H, W >= 1, both >= 2 with pool planes; x, the planes and proj_w 16-byte aligned; no output may overlap an input or
 *   another output.
 *
 * crg_hed_fuse: HEDdetector's tail (:73-77) in one launch.  maps: HOST array of n_maps (1..8) device pointers to fp32 side maps
 *   [N][map_h[i]][map_w[i]] (dense; map_h, map_w host arrays, all read when the call is made).  Per output pixel (x, y) and map, with the
 *   map's tables (sx, fx) = column x and (sy, fy) = row y, every operation rounded to fp32 on its own (no fused multiply-add):
 *     r(k) = s[k][sx] * (1 - fx) + s[k][min(sx + 1, w - 1)] * fx          for the rows k = sy and min(sy + 1, h - 1)
 *     u    = r(sy) * (1 - fy) + r(min(sy + 1, h - 1)) * fy                a map whose size is (H, W) is copied, its tables are not read
 *   mean = (((u_1 + u_2) + u_3) + ..) / (float)n_maps;  e = 1 / (1 + exp(-(double)mean));  out = (uint8) clip(e * 255.0, 0, 255), truncated.
 *   tab_idx int32 / tab_frac fp32, device: per map W column entries then H row entries, map i at i * (W + H); indices must lie inside
 *   their map (cremage_amd.postprocess.hed_tables builds them, in double, on the host).  out uint8 [N][H][W]; mean fp32 [N][H][W] or
 *   NULL.  Errors (-22, before any launch): n_maps outside 1..8, an empty size, an output overlapping a map, the tables or the other output.
 * No allocation, no host synchronisation.  Profile slot of both: CRG_K_ELEMENTWISE. */
int crg_relu_pool_proj(crg_ctx* ctx, void* stream, const float* x, void* hi, void* lo, void* pool_hi, void* pool_lo, const float* proj_w,
                       const float* proj_bias, float* proj, int N, int H, int W, int C);
int crg_hed_fuse(crg_ctx* ctx, void* stream, int n_maps, const void* const* maps, const int* map_h, const int* map_w, const int* tab_idx,
                 const float* tab_frac, void* out, float* mean, int N, int H, int W);

#ifdef __cplusplus
}
#endif
#endif /* CRG_HIP_H */
