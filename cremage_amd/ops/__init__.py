"""Torch-facing wrappers over the C-ABI (libcrg_hip.so).

PyTorch is used here only as the allocator / stream owner (`torch.empty`, `data_ptr()`, `torch.cuda.current_stream()`); every arithmetic
op on the hot path is a hand-written HIP kernel reached through `cremage_amd._lib`.  There is deliberately no CPU or eager fallback: a
CPU tensor, an unsupported shape or a missing library raises.

Layout contract: image activations are 4-D tensors with logical shape [N, C, H, W] and `torch.channels_last` strides (physically NHWC),
so the reference's hooks that index channels on dim 1 (ControlNet residual adds cldm.py:57-65, `th.cat(..., dim=1)` openaimodel.py:808)
keep working on them; token activations are contiguous [B, T, C].

Precision contract: bf16 activations -> CRG_PREC_BF16 kernels; fp32 activations -> CRG_PREC_BF16X3 (split-bf16, fp32-class) kernels.
Weights stay torch Parameters (any float dtype); their packed bf16 images are cached keyed on (data_ptr, _version, dtype, device, kind)
so that `load_state_dict`, LoRA `setattr` (image_generator.py:408-453) and `.to()/.half()` invalidate them.

One module per kernel family, each built on `_base` and on the families it composes (conv -> gemm -> norms -> packing / side_channels),
never the other way round; this package re-exports their public names.  The dev knobs live in `cremage_amd.knobs`, not here.
"""
from .. import knobs  # noqa: F401  (`ops.knobs` is the module itself; no knob is copied into this namespace)
# (underscore names: the launch plumbing and the statistics side channel, for tests that call an entry point of the library directly)
from ._base import (HALF, TensorKeyedCache, _h, _st, clear_weight_cache, empty_image, f32_vec, image_of, image_of_stats,  # noqa: F401
                    nchw_to_nhwc, nhwc_to_nchw, profile, to_channels_last, tokens_of)
from .annot import HED_MAX_MAPS, hed_fuse, relu_pool_proj
from .attn import attention, attention_rows_v, attention_x3_ok
from .conv import affine_cast, conv1x1, conv2d, mx_conv_ok, split_bf16, upsample_subpixel_ok
from .film import avg_pool2, flow_up2_add, leaky_split, scale_into, warp_flow
from .frames import MAX_FRAMES, add_frames, attention_frames, blend_frames, conv_frames, conv_frames_thin, conv_frames_x3, frames_weight, lincomb_frames
from .gemm import _gemm, last_route, linear, linear_transposed, linear_transposed_ok, ln_linear, ln_linear_auto, ln_linear_ok, rows_per_sample  # noqa: F401
from .imaging import (BLEND_GRAY, RESAMPLE_BITS, bilinear_tables, blur_blend_u8, lanczos_tables, paste_warped_u8, poisson_clone, poisson_tables, resample_u8,
                      upscale_noise, upscaled_size, warp_affine_u8)
from .mx8 import dequant_mx8_host, ff_mx8_ok, linear_mx8, linear_mx8_host, packed_weight_mx8, quant_mx8, quant_mx8_host
from .norms import group_norm, layer_norm, softmax_rows_
from .packing import MX_X_LOG2, packed_geglu_bias, packed_ln_weight, packed_weight, packed_weight_mx, split_mx
from .side_channels import (GN_STATS_MIN_HW, _gn_rows_of, _gn_stats_of, attach_time_rows, dup_batch, ln_epi_ok, ln_epi_wanted,  # noqa: F401
                            mark_cfg_dup, row_stats_parts, time_rows_of)
from .unblur import conv_transpose2d, group_norm_add_act
from .steps import KSTEP_KINDS, STEP_KINDS, axpby_, cfg_ddim_step_, cfg_dpmpp2m_step_, cfg_euler_step_, cfg_kstep_, cfg_sampler_step_, silu, timestep_embedding

__all__ = [
    "BLEND_GRAY", "GN_STATS_MIN_HW", "HALF", "HED_MAX_MAPS", "KSTEP_KINDS", "MAX_FRAMES", "MX_X_LOG2", "RESAMPLE_BITS", "STEP_KINDS", "TensorKeyedCache", "add_frames",
    "affine_cast", "attach_time_rows", "attention", "attention_frames", "attention_rows_v", "attention_x3_ok", "avg_pool2", "axpby_", "bilinear_tables",
    "blend_frames", "blur_blend_u8", "cfg_ddim_step_", "cfg_dpmpp2m_step_", "cfg_euler_step_", "cfg_kstep_", "cfg_sampler_step_", "clear_weight_cache",
    "conv1x1", "conv2d", "conv_transpose2d", "conv_frames", "conv_frames_thin", "conv_frames_x3", "dequant_mx8_host", "dup_batch", "empty_image", "f32_vec", "ff_mx8_ok",
    "flow_up2_add", "frames_weight", "group_norm", "group_norm_add_act", "hed_fuse", "image_of", "image_of_stats", "lanczos_tables", "last_route", "layer_norm", "leaky_split",
    "lincomb_frames", "linear", "linear_mx8", "linear_mx8_host", "linear_transposed", "linear_transposed_ok", "ln_epi_ok", "ln_epi_wanted", "ln_linear",
    "ln_linear_auto", "ln_linear_ok", "mark_cfg_dup", "mx_conv_ok", "nchw_to_nhwc", "nhwc_to_nchw", "packed_geglu_bias", "packed_ln_weight",
    "packed_weight", "packed_weight_mx", "packed_weight_mx8", "paste_warped_u8", "poisson_clone", "poisson_tables", "profile", "quant_mx8", "quant_mx8_host",
    "relu_pool_proj", "resample_u8", "row_stats_parts", "rows_per_sample", "scale_into", "silu", "softmax_rows_", "split_bf16", "split_mx", "time_rows_of",
    "timestep_embedding", "to_channels_last", "tokens_of", "upsample_subpixel_ok", "upscale_noise", "upscaled_size", "warp_affine_u8", "warp_flow",
]
