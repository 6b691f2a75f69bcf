"""What rides on tensor objects next to their data: GroupNorm statistics, LayerNorm row statistics, the CFG-duplicate mark, time rows."""
from typing import Optional

import torch

from .. import knobs
from ._base import HALF, to_channels_last

# ---------------------------------------------------------------------------------- GroupNorm statistics side channel
# A conv / linear whose output feeds a GroupNorm can write, next to its output, the per-(32-row block, channel) sum and sum of
# squares of what it stored (crg_conv_args.gn_stats / crg_gemm_args.gn_stats).  The buffer rides on the returned tensor object as
# `_crg_gn = (stats, version, rows per sample[, rows per partial])`; group_norm() uses it when the tensor has not been written since
# (`_version`: ControlNet's in-place residual adds, cldm.py:57-65, invalidate it) and then skips its statistics pass over the tensor.
GN_STATS_MIN_HW = 512  # smaller images take the single-launch GroupNorm kernel, which reads the tensor once anyway


def _gn_stats_buffer(rows: int, cols: int, hw: Optional[int], in_dtype, out_dtype, device) -> Optional[torch.Tensor]:
    if not knobs.GN_STATS or not hw or hw % 32 or hw < GN_STATS_MIN_HW or rows % hw or cols % 8:
        return None
    if in_dtype != HALF or out_dtype not in (HALF, torch.float32):  # fp32 outputs: the fp32-class conv on split planes (VAE)
        return None
    return torch.empty((2, (rows + 31) // 32, cols), dtype=torch.float32, device=device)


def _gn_stats_of(t: torch.Tensor, hw: int) -> Optional[torch.Tensor]:
    g = getattr(t, "_crg_gn", None)
    if g is None or g[1] != t._version or g[2] != hw or g[0].shape[2] != t.shape[1]:
        return None
    return g[0]


def _gn_rows_of(t: Optional[torch.Tensor]) -> int:
    """Rows per partial of the statistics riding on t (32 unless the producer said otherwise)."""
    g = getattr(t, "_crg_gn", None) if t is not None else None
    return int(g[3]) if (g is not None and len(g) > 3) else 32


# ---------------------------------------------------------------------------------- LayerNorm as a GEMM epilogue
# nn.LayerNorm in front of a Linear (attention.py:900-912) never runs as a launch of its own when the LayerNorm's INPUT was written by a
# GEMM of this library: that producer hands over per-row (sum, sum of squares) partials (crg_gemm_args.row_stats, riding on the
# tensor as `_crg_ln = (stats, version)` like the GroupNorm channel above), and the consuming GEMM runs on the raw rows with W o gamma
# and corrects its accumulators in the epilogue (crg_gemm_args.ln_stats).  Any width K; the K = 320 row-resident kernel (crg_ln_gemm)
# stays the route of the 64x64 level unless knobs.LN_EPI_320 says otherwise.
def row_stats_parts(n: int) -> int:
    """Column partials per row the producer writes for an N-wide output (include/crg_hip.h: 2 * ceil(N / tile), tile 160 | 128)."""
    bn = 160 if n % 160 == 0 else 128
    return 2 * ((n + bn - 1) // bn)


def ln_epi_wanted(width: int, geglu: bool = False) -> bool:
    """Should the producer of a LayerNorm input of this width emit row statistics - would its consumer (the GEGLU projection if `geglu`,
    else a plain projection) use them?"""
    return knobs.LN_EPI and bool(knobs.LN_EPI_MASK & (2 if geglu else 1)) and row_stats_parts(width) <= 16 and (width != 320 or knobs.LN_EPI_320 >= (2 if geglu else 1))


def _ln_stats_of(x: torch.Tensor) -> Optional[torch.Tensor]:
    g = getattr(x, "_crg_ln", None)
    K = x.shape[-1]
    if g is None or g[1] != x._version or g[0].shape[0] != x.numel() // K or g[0].shape[1] != row_stats_parts(K) or g[0].shape[1] > 16:
        return None
    return g[0]


def ln_epi_ok(x: torch.Tensor, weight: torch.Tensor, act: Optional[str] = None) -> bool:
    """Can `linear(x, weight, ..., ln=...)` run - does x carry valid row statistics and does the GEMM take the shape?"""
    if not (knobs.LN_EPI and x.is_cuda and x.dtype == HALF and x.is_contiguous() and act in (None, "geglu")) or not (knobs.LN_EPI_MASK & (2 if act == "geglu" else 1)):
        return False
    K = x.shape[-1]
    N = weight.shape[0]
    if weight[0].numel() != K or K % 8 or N % (32 if act == "geglu" else 8):
        return False
    if K == 320 and knobs.LN_EPI_320 < (2 if act == "geglu" else 1):
        return False
    return _ln_stats_of(x) is not None


# ---------------------------------------------------------------------------------- CFG-shared prefix
# Classifier-free guidance by batch doubling (ldm_wrapper_for_k_diffusion.py:67-93) hands the UNet cat([x] * 2) with cat([t] * 2): until
# the first cross-attention reads the (different) conditioning of the two halves, both halves compute the same values.  The sampler
# wrapper of this package marks such an input (never inferred from data); the UNet then runs that prefix on one half and duplicates
# the activations where the halves start to differ.  knobs.CFG_SHARE = False runs the whole batch as before.
def mark_cfg_dup(x: torch.Tensor) -> torch.Tensor:
    """Caller's promise: x == cat([h, h]) along the batch dim and so are the timesteps that go with it."""
    x._crg_cfg_dup = True
    return x


def dup_batch(t: torch.Tensor) -> torch.Tensor:
    """cat([t, t], dim 0) of a token tensor [B, T, C] or of a channels-last image (strides kept); one copy kernel.  The GroupNorm
    statistics riding on an image (32-row blocks, sample-major) are duplicated with it."""
    if t.dim() == 4:
        v = t.permute(0, 2, 3, 1)
        if not v.is_contiguous():
            v = to_channels_last(t).permute(0, 2, 3, 1)
        out = torch.cat([v, v], 0).permute(0, 3, 1, 2)
        g = getattr(t, "_crg_gn", None)
        if g is not None and g[1] == t._version:
            rows = g[3] if len(g) > 3 else 32
            if rows == 32:
                st = torch.cat([g[0], g[0]], 1)
            else:  # tile partials: the first M / rows partials of each plane, sample-major; the plane stride stays that of the 32-row layout
                used = g[0].shape[1] * 32 // rows
                st = torch.empty((2, 2 * g[0].shape[1], g[0].shape[2]), dtype=g[0].dtype, device=g[0].device)
                st[:, :used] = g[0][:, :used]
                st[:, used:2 * used] = g[0][:, :used]
            out._crg_gn = (st, out._version, g[2], rows)
        return out
    t = t.contiguous()
    return torch.cat([t, t], 0)


# ---------------------------------------------------------------------------------- hoisted timestep work
# What a UNet call computes from the timestep alone (sinusoid -> time_embed MLP -> SiLU -> the ResBlocks' emb_layers, openaimodel.py:793-796,
# :222-228) is known for the whole schedule before the first step.  A sampler of this package computes it once (`UNetModel.time_rows`) and
# hands each step its rows on the timestep tensor, which the reference's containers pass on untouched (ddpm.py:1034, :1517-1519) like the
# CFG mark above.  The rows name the network they were computed with: a ControlNet that receives the same timesteps ignores them.
# knobs.TIME_ROWS = False computes the embedding inside every call as before.
def attach_time_rows(timesteps: torch.Tensor, rows: torch.Tensor, owner) -> torch.Tensor:
    """Caller's promise: rows == owner.time_rows(timesteps[None])[0] ([N, sum Cout] fp32 of `owner`, a UNetModel)."""
    timesteps._crg_time_rows = (owner, rows)
    return timesteps


def time_rows_of(timesteps, owner):
    """The rows attached for `owner`, or None."""
    tr = getattr(timesteps, "_crg_time_rows", None)
    return tr[1] if (knobs.TIME_ROWS and tr is not None and tr[0] is owner) else None
