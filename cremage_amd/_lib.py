"""ctypes binding of libcrg_hip.so (include/crg_hip.h).

The product path has NO fallback: if the library is missing or a call fails, a Python exception
is raised (the reference's ML process has no handler, modules/cremage/mp/mp.py:125, so clean
exceptions - never aborts - are the contract).
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# CRG_LIB: developer override used for A/B runs of two builds on the same GPU box (tools/); the default is the in-tree build
# CRG_HALF=f16: the fp16-operand build of the same kernels (libcrg_hip_f16.so); activations / packed weights are torch.float16 then
HALF_F16 = os.environ.get("CRG_HALF", "bf16").lower() in ("f16", "fp16", "float16", "half")
LIB_PATH = os.path.abspath(os.environ["CRG_LIB"]) if os.environ.get("CRG_LIB") else os.path.join(_HERE, "libcrg_hip_f16.so" if HALF_F16 else "libcrg_hip.so")

BF16, F32, F16 = 0, 1, 2
PREC_BF16, PREC_BF16X3, PREC_F16MX = 0, 1, 2
EPI_NONE, EPI_SILU, EPI_GEGLU = 0, 1, 2
BIAS_NONE, BIAS_COL, BIAS_ROW = 0, 1, 2
PACK_LINEAR, PACK_CONV, PACK_GEGLU, PACK_CONV_UP2, PACK_CONVT_UP2 = 0, 1, 2, 3, 4
K_SLOTS = 17  # enum crg_kernel_slot
SLOT_NAMES = ["gemm_w1", "gemm_w4", "gemm_w5", "gemm_x3", "conv_w1", "conv_w4", "conv_w5", "conv_x3", "splitk_reduce", "attention",
              "gn_stats", "gn_apply", "layernorm", "elementwise", "conv_small", "softmax", "lngemm"]
SLOT_FAMILY = ["gemm", "gemm", "gemm", "gemm", "conv", "conv", "conv", "conv", "splitk_reduce", "attention", "groupnorm", "groupnorm",
               "layernorm", "elementwise", "conv_small", "softmax", "gemm"]

c_void_p, c_int, c_int64, c_float, c_size_t = C.c_void_p, C.c_int, C.c_int64, C.c_float, C.c_size_t


class GemmArgs(C.Structure):
    _fields_ = [
        ("a", c_void_p), ("lda", c_int64), ("a_bstride", c_int64),
        ("w", c_void_p), ("ldw", c_int64), ("w_bstride", c_int64),
        ("w_lo", c_void_p),
        ("bias", c_void_p), ("bias_mode", c_int),
        ("residual", c_void_p), ("ldr", c_int64), ("r_bstride", c_int64),
        ("y", c_void_p), ("ldy", c_int64), ("y_bstride", c_int64),
        ("M", c_int), ("N", c_int), ("K", c_int), ("batch", c_int),
        ("epilogue", c_int),
        ("a_dtype", c_int), ("y_dtype", c_int), ("prec", c_int),
        ("a_is_weight", c_int),
        ("a_lo", c_void_p),
        ("gn_stats", c_void_p),
        ("vt", c_void_p), ("vt_n0", c_int), ("vt_tokens", c_int), ("vt_ld", c_int64),
        ("row_stats", c_void_p), ("row_stats_parts", c_int),
        ("ln_stats", c_void_p), ("ln_parts", c_int), ("ln_colsum", c_void_p), ("ln_eps", c_float),
        ("rows_per_sample", c_int),
    ]


class LnGemmArgs(C.Structure):
    _fields_ = [
        ("x", c_void_p), ("ldx", c_int64),
        ("gamma", c_void_p), ("beta", c_void_p), ("eps", c_float),
        ("w", c_void_p), ("ldw", c_int64),
        ("bias", c_void_p),
        ("y", c_void_p), ("ldy", c_int64),
        ("M", c_int), ("N", c_int), ("K", c_int),
        ("epilogue", c_int),
        ("vt", c_void_p), ("vt_n0", c_int), ("vt_tokens", c_int), ("vt_ld", c_int64),
        ("residual", c_void_p), ("ldr", c_int64),
    ]


class ConvArgs(C.Structure):
    _fields_ = [
        ("x", c_void_p), ("x2", c_void_p), ("C1", c_int), ("C2", c_int),
        ("w", c_void_p), ("w_lo", c_void_p),
        ("bias", c_void_p), ("cvec", c_void_p),
        ("cvec_ld", c_int64),
        ("residual", c_void_p),
        ("y", c_void_p),
        ("N", c_int), ("H", c_int), ("W", c_int), ("Cout", c_int), ("Ho", c_int), ("Wo", c_int),
        ("ksize", c_int), ("stride", c_int), ("pad_t", c_int), ("pad_l", c_int),
        ("upsample2x", c_int),
        ("x_dtype", c_int), ("y_dtype", c_int), ("prec", c_int),
        ("x_lo", c_void_p),
        ("gn_stats", c_void_p),
        ("gn_gamma", c_void_p), ("gn_beta", c_void_p), ("gn_y", c_void_p),
        ("gn_groups", c_int), ("gn_silu", c_int), ("gn_eps", C.c_float),
        ("mx_log2", c_int * 4),
        ("gn_stats_rows", C.POINTER(c_int)),
    ]


STEP_EULER_A, STEP_HEUN_1, STEP_HEUN_2, STEP_DPMPP2S_1, STEP_DPMPP2S_2, STEP_LMS = range(6)  # CRG_STEP_*


class SamplerStepArgs(C.Structure):
    _fields_ = [
        ("kind", c_int), ("n", c_int64),
        ("x", c_void_p), ("eps", c_void_p), ("x2", c_void_p), ("d", c_void_p), ("hist", c_void_p * 3), ("noise", c_void_p),
        ("c_out", c_float), ("cfg_scale", c_float), ("sigma", c_float), ("dt", c_float), ("sigma_up", c_float), ("s_noise", c_float),
        ("m", c_float * 4), ("coef", c_float * 4),
        ("n_hist", c_int), ("one_call", c_int), ("add_noise", c_int),
    ]


KSTEP_DPM2_2, KSTEP_SDE_1, KSTEP_SDE_2M, KSTEP_SDE_3M = range(4)  # CRG_KSTEP_*


class KStepArgs(C.Structure):
    _fields_ = [
        ("kind", c_int), ("n", c_int64),
        ("x", c_void_p), ("eps", c_void_p), ("x2", c_void_p), ("den_out", c_void_p), ("old", c_void_p * 2), ("noise", c_void_p),
        ("c_out", c_float), ("cfg_scale", c_float), ("sigma", c_float), ("dt", c_float), ("sigma_up", c_float), ("s_noise", c_float),
        ("m", c_float * 2), ("a", c_float), ("c1", c_float), ("c2", c_float), ("p", c_float * 2),
        ("r", c_float * 2), ("rsum", c_float), ("phi2", c_float), ("phi3", c_float),
        ("order", c_int), ("last", c_int), ("have_old", c_int), ("add_noise", c_int),
    ]


class ResampleArgs(C.Structure):
    _fields_ = [
        ("src", c_void_p), ("src_u8", c_int),
        ("src_sn", c_int64), ("src_sc", c_int64), ("src_sy", c_int64), ("src_sx", c_int64),
        ("src_h", c_int), ("src_w", c_int),
        ("x0", c_int), ("y0", c_int), ("w", c_int), ("h", c_int),
        ("N", c_int), ("C", c_int),
        ("W", c_int), ("H", c_int),
        ("kx", c_void_p), ("x_bounds", c_void_p), ("ksize_x", c_int),
        ("ky", c_void_p), ("y_bounds", c_void_p), ("ksize_y", c_int),
        ("dst", c_void_p), ("dst_u8", c_int),
        ("dst_sn", c_int64), ("dst_sc", c_int64), ("dst_sy", c_int64), ("dst_sx", c_int64),
        ("dst_h", c_int), ("dst_w", c_int),
        ("ox", c_int), ("oy", c_int),
        ("out_a", c_float), ("out_b", c_float),
        ("fill", c_int), ("fill_value", c_float),
    ]


class PoissonArgs(C.Structure):
    _fields_ = [
        ("image", c_void_p),
        ("img_sn", c_int64), ("img_sc", c_int64), ("img_sy", c_int64), ("img_sx", c_int64),
        ("img_h", c_int), ("img_w", c_int),
        ("patch", c_void_p),
        ("pat_sn", c_int64), ("pat_sc", c_int64), ("pat_sy", c_int64), ("pat_sx", c_int64),
        ("N", c_int),
        ("h", c_int), ("w", c_int),
        ("x", c_int), ("y", c_int),
        ("margin", c_int),
        ("s_rows", c_void_p), ("s_cols", c_void_p), ("rden", c_void_p),
        ("work", c_void_p), ("field", c_void_p),
    ]


class BlendArgs(C.Structure):
    _fields_ = [
        ("original", c_void_p), ("org_sn", c_int64), ("org_sy", c_int64), ("org_sx", c_int64),
        ("updated", c_void_p), ("upd_sn", c_int64), ("upd_sy", c_int64), ("upd_sx", c_int64),
        ("mask", c_void_p), ("msk_sn", c_int64), ("msk_sy", c_int64), ("msk_sx", c_int64),
        ("gray_mode", c_int),
        ("out", c_void_p), ("out_sn", c_int64), ("out_sy", c_int64), ("out_sx", c_int64),
        ("N", c_int), ("H", c_int), ("W", c_int), ("C", c_int),
        ("win_x", c_int), ("win_y", c_int), ("win_w", c_int), ("win_h", c_int),
        ("taps", C.c_double * 11),
    ]


MX8_OUT_HALF, MX8_OUT_F32, MX8_OUT_MX8 = 0, 1, 2  # enum crg_mx8_out


class Mx8GemmArgs(C.Structure):
    _fields_ = [
        ("a_q", c_void_p), ("lda", c_int64),
        ("a_e", c_void_p), ("lde", c_int64),
        ("w_q", c_void_p), ("w_e", c_void_p),
        ("bias", c_void_p),
        ("residual", c_void_p), ("ldr", c_int64),
        ("y", c_void_p), ("ldy", c_int64),
        ("y_e", c_void_p), ("ldye", c_int64),
        ("M", c_int), ("N", c_int), ("K", c_int),
        ("epilogue", c_int),
        ("y_kind", c_int),
    ]


class AttnX3Args(C.Structure):
    _fields_ = [
        ("q", c_void_p), ("ldq", c_int64),
        ("k", c_void_p), ("ldk", c_int64),
        ("vt", c_void_p), ("ldvt", c_int64),
        ("o", c_void_p), ("ldo", c_int64),
        ("B", c_int), ("H", c_int), ("Nq", c_int), ("Nk", c_int), ("Dh", c_int),
        ("scale", c_float),
    ]


class ConvFramesArgs(C.Structure):
    _fields_ = [
        ("x", c_void_p), ("w", c_void_p),
        ("bias", c_void_p),
        ("cvec", c_void_p), ("cvec_ld", c_int64),
        ("residual", c_void_p), ("rscale", c_void_p),
        ("y", c_void_p),
        ("b", c_int), ("T", c_int), ("S", c_int), ("Cin", c_int), ("Cout", c_int),
    ]


class ConvFramesX3Args(C.Structure):
    _fields_ = [
        ("x_hi", c_void_p), ("x_lo", c_void_p),
        ("w_hi", c_void_p), ("w_lo", c_void_p),
        ("bias", c_void_p),
        ("cvec", c_void_p), ("cvec_ld", c_int64),
        ("residual", c_void_p), ("rscale", c_void_p),
        ("y", c_void_p),
        ("b", c_int), ("T", c_int), ("S", c_int), ("Cin", c_int), ("Cout", c_int),
    ]


class FilmWarpArgs(C.Structure):
    _fields_ = [
        ("src", c_void_p), ("ld_src", c_int64),
        ("flow", c_void_p), ("ld_flow", c_int64),
        ("scale", c_void_p),
        ("dst", c_void_p), ("ld_dst", c_int64),
        ("hi", c_void_p), ("lo", c_void_p), ("ld_planes", c_int64),
        ("N", c_int), ("H", c_int), ("W", c_int), ("C", c_int),
    ]


class FilmActArgs(C.Structure):
    _fields_ = [
        ("x", c_void_p), ("ld_x", c_int64),
        ("y", c_void_p), ("ld_y", c_int64),
        ("hi", c_void_p), ("lo", c_void_p), ("ld_planes", c_int64),
        ("pool", c_void_p), ("ld_pool", c_int64),
        ("scale", c_void_p),
        ("N", c_int), ("H", c_int), ("W", c_int), ("C", c_int),
        ("slope", c_float),
    ]


class AttnFramesArgs(C.Structure):
    _fields_ = [
        ("q", c_void_p), ("ldq", c_int64),
        ("k", c_void_p), ("ldk", c_int64),
        ("v", c_void_p), ("ldv", c_int64),
        ("o", c_void_p), ("ldo", c_int64),
        ("b", c_int), ("T", c_int), ("S", c_int), ("H", c_int), ("Dh", c_int),
        ("scale", c_float),
        ("dtype", c_int),
    ]


ROUTE_KERNELS = ["none", "glds", "rowhalo", "conv_pp", "gemm_ring", "gemm_reg", "planes", "convt"]  # enum crg_route_kernel
ROUTE_REDUCES = ["none", "plain", "stats", "rows", "gn"]  # enum crg_route_reduce


class Route(C.Structure):
    _fields_ = [("kernel", c_int), ("wnt", c_int), ("config", c_int), ("splits", c_int), ("tail_splits", c_int), ("rowhalo", c_int),
                ("halo_lin", c_int), ("pair", c_int), ("up2", c_int), ("mx", c_int), ("reduce", c_int), ("gn_stats_rows", c_int)]


class Profile(C.Structure):
    _fields_ = [("ms", C.c_double * K_SLOTS), ("flops", C.c_double * K_SLOTS), ("bytes", C.c_double * K_SLOTS),
                ("launches", C.c_int64 * K_SLOTS)]


# name -> (restype, argtypes); every symbol include/crg_hip.h declares
SIGNATURES = {
    "crg_version": (c_int, []),
    "crg_half_kind": (c_int, []),
    "crg_ctx_create": (c_int, [c_int, C.POINTER(c_void_p)]),
    "crg_ctx_destroy": (None, [c_void_p]),
    "crg_last_error": (C.c_char_p, [c_void_p]),
    "crg_ctx_reserve": (c_int, [c_void_p, c_size_t]),
    "crg_ctx_set_invariant": (c_int, [c_void_p, c_int]),
    "crg_ctx_get_invariant": (c_int, [c_void_p]),
    "crg_kernel_name": (C.c_char_p, [c_int]),
    "crg_profile_begin": (c_int, [c_void_p]),
    "crg_profile_end": (c_int, [c_void_p, c_void_p, C.POINTER(Profile)]),
    "crg_groupnorm": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int,
                              c_int, c_float, c_int, c_int]),
    "crg_groupnorm_split": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int,
                                    c_int, c_float, c_int]),
    "crg_groupnorm_pre_split": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int,
                                        c_float, c_int]),
    "crg_groupnorm_pre": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int,
                                  c_int, c_int, c_float, c_int, c_int, c_int, c_int]),
    "crg_split_bf16": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int64]),
    "crg_split_mx": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int, c_int, c_int]),
    "crg_groupnorm_mx": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_float,
                                 c_int, c_int, c_int]),
    "crg_pack_weight_mx": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_int, c_int]),
    "crg_layernorm": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int, c_float, c_int]),
    "crg_gemm": (c_int, [c_void_p, c_void_p, C.POINTER(GemmArgs)]),
    "crg_conv2d": (c_int, [c_void_p, c_void_p, C.POINTER(ConvArgs)]),
    "crg_last_route": (c_int, [c_void_p, C.POINTER(Route)]),
    "crg_ln_gemm": (c_int, [c_void_p, c_void_p, C.POINTER(LnGemmArgs)]),
    "crg_pack_weight": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_void_p, c_void_p]),
    "crg_pack_geglu_bias": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_void_p]),
    "crg_pack_ln_weight": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_void_p, c_void_p, c_void_p]),
    "crg_attention": (c_int, [c_void_p, c_void_p, c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_int64,
                              c_int, c_int, c_int, c_int, c_int, c_float, c_int]),
    "crg_attention_v": (c_int, [c_void_p, c_void_p, c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_int64,
                              c_int, c_int, c_int, c_int, c_int, c_float, c_int]),
    "crg_softmax_rows": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int, c_int64, c_float, c_int]),
    "crg_conv_small": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int,
                               c_int, c_int, c_int]),
    "crg_timestep_embedding": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int]),
    "crg_silu": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int]),
    "crg_nchw_to_nhwc": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int]),
    "crg_nhwc_to_nchw": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int]),
    "crg_nchw2_to_nhwc": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int]),
    "crg_cfg_euler_step": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_float, c_float, c_float, c_float]),
    "crg_cfg_ddim_step": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_float, c_float, c_float, c_float, c_float,
                                  c_float]),
    "crg_cfg_dpmpp2m_step": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_float, c_float, c_float, c_float, c_float,
                                     c_float, c_int]),
    "crg_cfg_sampler_step": (c_int, [c_void_p, c_void_p, C.POINTER(SamplerStepArgs)]),
    "crg_cfg_kstep": (c_int, [c_void_p, c_void_p, C.POINTER(KStepArgs)]),
    "crg_resize_noise": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int, c_int, c_int, c_int, c_void_p, c_void_p,
                                 c_void_p, c_void_p, c_float, c_float, c_float]),
    "crg_resample_u8": (c_int, [c_void_p, c_void_p, C.POINTER(ResampleArgs)]),
    "crg_poisson_clone": (c_int, [c_void_p, c_void_p, C.POINTER(PoissonArgs)]),
    "crg_blur_blend_u8": (c_int, [c_void_p, c_void_p, C.POINTER(BlendArgs)]),
    "crg_axpby": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_float, c_float, c_int]),
    "crg_affine_cast": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_float, c_float, c_float, c_float, c_int,
                                c_int]),
    "crg_quant_mx8": (c_int, [c_void_p, c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_int64, c_int]),
    "crg_pack_weight_mx8": (c_int, [c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_void_p, c_void_p]),
    "crg_gemm_mx8": (c_int, [c_void_p, c_void_p, C.POINTER(Mx8GemmArgs)]),
    "crg_attention_x3": (c_int, [c_void_p, c_void_p, C.POINTER(AttnX3Args)]),
    "crg_conv_frames": (c_int, [c_void_p, c_void_p, C.POINTER(ConvFramesArgs)]),
    "crg_attention_frames": (c_int, [c_void_p, c_void_p, C.POINTER(AttnFramesArgs)]),
    "crg_add_frames": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int, c_int, c_int]),
    "crg_lincomb_frames": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_int]),
    "crg_conv_frames_x3": (c_int, [c_void_p, c_void_p, C.POINTER(ConvFramesX3Args)]),
    "crg_conv_frames_thin": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int]),
    "crg_film_warp": (c_int, [c_void_p, c_void_p, C.POINTER(FilmWarpArgs)]),
    "crg_film_pool2": (c_int, [c_void_p, c_void_p, c_void_p, c_int64, c_void_p, c_int64, c_int, c_int, c_int, c_int]),
    "crg_film_flow_up": (c_int, [c_void_p, c_void_p, c_void_p, c_int64, c_void_p, c_int64, c_void_p, c_int64, c_int, c_int, c_int]),
    "crg_film_act": (c_int, [c_void_p, c_void_p, C.POINTER(FilmActArgs)]),
    "crg_conv_transpose2d": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int, c_int, c_int]),
    "crg_groupnorm_add_act": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_void_p, c_void_p, c_void_p, c_void_p, c_int64, c_void_p, c_void_p,
                                      c_int64, c_void_p, c_int64, c_int, c_int, c_int, c_int, c_float, c_int]),
    "crg_warp_affine_u8": (c_int, [c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_int, c_int, c_int, C.POINTER(C.c_double), c_int, c_void_p, c_int,
                                   c_int64, c_int64, c_int64, c_int64, c_int, c_int]),
    "crg_paste_warped_u8": (c_int, [c_void_p, c_void_p, c_void_p, c_int64, c_int64, c_int, c_int, c_int, c_void_p, c_int, c_int64, c_int64, c_int64,
                                    c_int, c_int, C.POINTER(C.c_double), c_int, c_int, c_int, c_int]),
    "crg_relu_pool_proj": (c_int, [c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_void_p, c_int, c_int, c_int, c_int]),
    "crg_hed_fuse": (c_int, [c_void_p, c_void_p, c_int, C.POINTER(c_void_p), C.POINTER(c_int), C.POINTER(c_int), c_void_p, c_void_p, c_void_p, c_void_p,
                             c_int, c_int, c_int]),
}


class CrgError(RuntimeError):
    pass


_lib = None


def load():
    """dlopen the library and bind every declared symbol; raises if anything is missing."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise CrgError(f"{LIB_PATH} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                       "(cremage_amd has no CPU or PyTorch fallback)")
    import torch  # noqa: F401  (before the dlopen: the library must resolve the HIP runtime to the one PyTorch loads; with the system
    #                             runtime loaded first the process ends up with two, and the one behind this library sees no device)
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)  # AttributeError if the symbol is not exported
        fn.restype = res
        fn.argtypes = args
    if lib.crg_version() != 104:
        raise CrgError(f"libcrg_hip.so version {lib.crg_version()} does not match the binding (104)")
    if lib.crg_half_kind() != (1 if HALF_F16 else 0):
        raise CrgError(f"{LIB_PATH} computes in {'fp16' if lib.crg_half_kind() else 'bf16'} but CRG_HALF asks for {'fp16' if HALF_F16 else 'bf16'}")
    _lib = lib
    return lib


_ctxs = {}
_lane = 0


# ---- batch-invariant mode (crg_ctx_set_invariant; cremage_amd.set_batch_invariant is the public switch) ----
def parse_invariant(value, what="set_batch_invariant"):
    """tune_samples as the library takes it: None / 0 -> 0 (off), a positive integer -> itself.  A bool, a negative number or a
    non-integer is a ValueError."""
    if value is None:
        return 0
    if isinstance(value, bool) or not isinstance(value, int):
        raise ValueError(f"{what}: tune_samples must be None or a non-negative integer, got {value!r}")
    if value < 0 or value >= 1 << 31:
        raise ValueError(f"{what}: tune_samples must be None or a non-negative integer below 2^31, got {value!r}")
    return int(value)


def parse_invariant_env(text):
    """CRG_BATCH_INVARIANT=<n>: empty / unset -> 0 (off), a decimal non-negative integer -> itself; anything else is a ValueError."""
    if text is None or text.strip() == "":
        return 0
    t = text.strip()
    if not t.isdigit():
        raise ValueError(f"CRG_BATCH_INVARIANT={text!r}: a non-negative integer expected (0 = off)")
    return parse_invariant(int(t), "CRG_BATCH_INVARIANT")


_invariant = parse_invariant_env(os.environ.get("CRG_BATCH_INVARIANT"))


def invariant() -> int:
    """tune_samples of the batch-invariant mode, 0 = off."""
    return _invariant


def set_invariant(tune_samples: int) -> None:
    """Set the mode on every live context and remember it for those created later (host bookkeeping, no launch)."""
    global _invariant
    _invariant = parse_invariant(tune_samples)
    for h in _ctxs.values():
        check(load().crg_ctx_set_invariant(h, _invariant), h, "crg_ctx_set_invariant")


def set_lane(i: int) -> int:
    """Select which of the device's contexts the following crg_* calls use.  A context owns scratch (split-K slabs, GroupNorm
    partials) and is not re-entrant, so work that runs CONCURRENTLY on several HIP streams needs one context per stream
    ("lane"); the single-stream caller never touches this.  Returns the previous lane."""
    global _lane
    prev, _lane = _lane, int(i)
    return prev


def ctx(device_index: int):
    """One context per (device, lane) (include/crg_hip.h: not re-entrant, single-threaded caller; lane 0 unless set_lane)."""
    key = (device_index, _lane)
    h = _ctxs.get(key)
    if h is None:
        lib = load()
        out = c_void_p()
        rc = lib.crg_ctx_create(device_index, C.byref(out))
        if rc != 0:
            raise CrgError(f"crg_ctx_create(device={device_index}) failed with {rc}: no usable HIP device")
        h = out
        if _invariant:
            check(lib.crg_ctx_set_invariant(h, _invariant), h, "crg_ctx_set_invariant")
        _ctxs[key] = h
    return h


def check(rc: int, h, what: str):
    if rc != 0:
        msg = load().crg_last_error(h)
        raise CrgError(f"{what} failed ({rc}): {msg.decode() if msg else '?'}")
