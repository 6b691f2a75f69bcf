"""Every Python-side dev knob of the package, once: a module global per knob, parsed from its CRG_* variable when this module is imported.

Readers look a knob up as `knobs.NAME` at the moment they need it (call time; for a captured graph that is capture time, see graphs.py),
so a test or a tool switches one by assigning `knobs.NAME` (`monkeypatch.setattr(knobs, "NAME", v)`).  Nothing copies a knob into another
module (`from .knobs import NAME` would go stale) and `cremage_amd.ops` does not re-export them.  Booleans parse as `value != "0"`, the two
LayerNorm integers as `int(value)`.  This module imports nothing but `os`.  Not here: CRG_HALF, CRG_LIB and CRG_BATCH_INVARIANT choose or
configure the library at import (_lib.py); the knobs the native code reads with getenv are listed in include/crg_hip.h.
"""
import os

# ---- GroupNorm statistics side channel (ops/side_channels.py; read by ops.linear / ops.conv2d when they allocate the buffer)
GN_STATS = os.environ.get("CRG_GN_STATS", "1") != "0"          # 0 = every GroupNorm computes its own statistics
VAE_GN_STATS = os.environ.get("CRG_VAE_GN_STATS", "1") != "0"  # 0 = the fp32-class convs emit no statistics (ops.conv2d)
# Round 4: a producer may report a coarser granularity than 32 rows (crg_conv_args.gn_stats_rows: one partial per 256-pixel tile and channel
# from the staggered 3x3 conv); the tuple carries it as a fourth element and crg_groupnorm_pre, given tile partials on every input, folds
# them inside the normalising launch - the finalise launch disappears.  0 (A/B): 32-row partials everywhere.  Read by ops.conv2d.
GN_TILE = os.environ.get("CRG_GN_TILE", "1") != "0"
# ---- LayerNorm as a GEMM epilogue (ops/side_channels.py: ln_epi_wanted / ln_epi_ok; ops.linear for row_stats)
LN_EPI = os.environ.get("CRG_LN_EPI", "1") != "0"  # (A/B) 0 = stand-alone layernorm launches as in round 3
# K = 320 (the 64x64 level, where crg_ln_gemm exists): 0 = row-resident kernel for every consumer (round 3), 1 (default) = the plain
# projections on the epilogue route (device time in a graph, tools/lnepi_probe.py: LN + Q | K | V 43.4 -> 40.6 us, LN + to_q 19.1 -> 16.6),
# the GEGLU projection stays row-resident (76.8 us against 95.7 on the epilogue route), 2 = the GEGLU projection as well
LN_EPI_320 = int(os.environ.get("CRG_LN_EPI_320", "1"))
LN_EPI_MASK = int(os.environ.get("CRG_LN_EPI_MASK", "3"))  # (A/B) bit 0 = plain consumers (Q | K | V, to_q) on the epilogue route, bit 1 = GEGLU consumers
# ---- opt-in precisions
# 1 = the VAE's ResnetBlock convs on MX planes (CRG_PREC_F16MX).  Correct and validated (tests/test_hip_ops.py::test_conv_mx) but measured
# 7-18 % slower than bf16 x 3 in round 4 (conv_rowhalo.hip, conv3_rowhalo_kernel<.., MX>: status note).  Read by ops.mx_conv_ok.
VAE_MX = os.environ.get("CRG_VAE_MX", "0") != "0"
# 1 = "mx8" is the default precision of newly built FeedForward modules (ldm_hip/transformer.py), a knob like CRG_VAE_MX; off, the MX8
# feed-forward runs only where FeedForward(precision="mx8") / cremage_amd.set_ff_precision asks for it
FF_MX8 = os.environ.get("CRG_FF_MX8", "0") != "0"
# 1 = fp32 attention goes through the flash kernel of the class (crg_attention_x3: one launch, no score buffer) wherever
# ops.attention_x3_ok holds.  Read per call of ops.attention, i.e. at CAPTURE time for a captured graph: a replay runs what was captured.
ATTN_X3_FLASH = os.environ.get("CRG_ATTN_X3", "0") != "0"
# fp32 score buffer of the unfused attention path (ops.attention processes queries in chunks that fit it); no environment variable,
# tests set it to force several chunks with a tail
SCORE_BUDGET_BYTES = 256 << 20
# ---- model-level sharing (A/B: 0 = as before the optimisation)
CFG_SHARE = os.environ.get("CRG_CFG_SHARE", "1") != "0"  # 0 = the UNet runs the whole CFG-doubled batch (ldm_hip/unet.py; ops/side_channels.py: mark_cfg_dup)
TIME_ROWS = os.environ.get("CRG_TIME_ROWS", "1") != "0"  # 0 = the timestep embedding is computed inside every UNet call (ops.time_rows_of, sampler_plan.py)
UP_SUBPIX = os.environ.get("CRG_UP_SUBPIX", "1") != "0"  # 0 = upsample convs keep the gather form (ops.upsample_subpixel_ok)
SELF_QKV = os.environ.get("CRG_SELF_QKV", "1") != "0"    # 0 = self-attention as fused Q|K GEMM + transposed-V GEMM, the round-1 form (ldm_hip/transformer.py)
# 0 = the fused sampler steps compute the CompVis wrapper's scalings and timestep per step (round 2) instead of once per run (samplers.py)
STEP_TABLES = os.environ.get("CRG_SAMPLER_TABLES", "1") != "0"
