"""The conv family: implicit-GEMM conv2d (16-bit, split-bf16 and MX planes), 1x1 convs, bf16 plane splitting and the affine cast."""
import ctypes as C
from typing import Optional

import torch

from .. import _lib as L, knobs
from ._base import (_DT, HALF, _act_dt, _call, _is_dense, _need_cuda, _p, _prec, empty_image, f32_vec, image_of_stats, to_channels_last, tokens_of)
from .gemm import linear
from .packing import MX_X_LOG2, packed_weight, packed_weight_mx
from .side_channels import _gn_stats_buffer


def affine_cast(x: torch.Tensor, a: float, b: float, dtype: torch.dtype, lo: float = float("-inf"), hi: float = float("inf")):
    """y = clamp(a*x + b, lo, hi) cast to `dtype`.  A dense x (contiguous, channels-last, any permutation) keeps its strides; a view
    with gaps or expanded dims is read through a compact copy in the same order of dims."""
    _need_cuda(x)
    if not _is_dense(x):
        x = x.clone(memory_format=torch.preserve_format)
        if not _is_dense(x):
            x = x.contiguous()
    y = torch.empty_strided(x.shape, x.stride(), dtype=dtype, device=x.device)
    _call("crg_affine_cast", x, _p(x), _p(y), x.numel(), a, b, lo, hi, _act_dt(x), _DT[dtype])
    return y


def split_bf16(x: torch.Tensor):
    """fp32 image -> (hi, lo) bf16 planes, hi = bf16(x), lo = bf16(x - hi): the fp32-class conv's operand format."""
    _need_cuda(x)
    x = to_channels_last(x)
    n, c, hh, ww = x.shape
    hi, lo = empty_image(n, c, hh, ww, HALF, x.device), empty_image(n, c, hh, ww, HALF, x.device)
    _call("crg_split_bf16", x, _p(x), _p(hi), _p(lo), x.numel())
    return hi, lo


def conv2d(x: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor] = None, stride: int = 1, padding=1,
           upsample2x: bool = False, x2: Optional[torch.Tensor] = None, cvec: Optional[torch.Tensor] = None,
           residual: Optional[torch.Tensor] = None, x_lo: Optional[torch.Tensor] = None, gn_stats: bool = False, gn=None,
           x_mx: Optional[torch.Tensor] = None, subpixel: Optional[bool] = None):
    """Implicit-GEMM conv over channels-last images.
    `gn` = (weight, bias, groups, eps, silu): also return silu?(GroupNorm(y)) - the norm that follows the conv inside a ResBlock
    (crg_conv_args.gn_y: on the small images of the two lowest UNet levels the launch that sums the K slices normalises as well);
    the call then returns (y, y_norm).  bf16 outputs only; anything else raises.
    padding: int (symmetric) or (top, left, bottom, right).  `upsample2x`: nearest-2x of the input is
    folded into the gather - or, where upsample_subpixel_ok() holds and nothing else is fused, run as four 2x2 parity convs on the source
    grid with pre-summed weights (4 / 9 of the multiplies).  `subpixel`: None = that form for fp32-class planes (`x_lo`) only, where
    rounding the fp32 sum of the taps is the format's own rounding; a 16-bit conv keeps the gather form unless the caller passes True and so
    accepts weights rounded to the operand type a second time (2e-3 of one conv's output); False = always the gather form.  `x2`: second half of a virtual channel concat.  `cvec` fp32 [N, Cout] is
    added per sample (timestep embedding); `residual` is added after.  `x_lo`: x is the bf16 hi plane of a pre-split
    fp32 activation and x_lo its lo plane (group_norm(split=True) / split_bf16): fp32-class conv with fp32 output.
    `gn_stats`: the output feeds a GroupNorm - emit its statistics side channel where the path supports it (bf16, side_channels.py).
    `x_mx`: x is the fp16 plane and x_mx the e4m3 pair plane of MX-split fp32 activations (split_mx / group_norm(split='mx')): the
    fp32-class conv on CRG_PREC_F16MX (3x3, stride 1, pad 1, Cin % 64 == 0; fp32 output)."""
    _need_cuda(x, weight, bias, x2, cvec, residual, x_lo, x_mx)
    if x_mx is not None:
        return _conv2d_mx(x, x_mx, weight, bias, stride, padding, upsample2x, x2, cvec, residual, x_lo, gn_stats, gn)
    x = to_channels_last(x)
    if x_lo is not None:
        x_lo = to_channels_last(x_lo)
        if x.dtype != HALF or x_lo.dtype != HALF or x_lo.shape != x.shape or x2 is not None:
            raise L.CrgError("conv2d: x / x_lo must be two bf16 planes of one shape (and no second input)")
    n, c1, hh, ww = x.shape
    c2 = 0
    if x2 is not None:
        x2 = to_channels_last(x2)
        c2 = x2.shape[1]
        if x2.shape[0] != n or x2.shape[2:] != x.shape[2:] or x2.dtype != x.dtype:
            raise L.CrgError("conv2d: concat halves disagree in shape/dtype")
    cout, cin, ks, _ = weight.shape
    if cin != c1 + c2:
        raise L.CrgError(f"conv2d: weight expects {cin} input channels, got {c1}+{c2}")
    pt, pl, pb, pr = (padding,) * 4 if isinstance(padding, int) else padding
    hv, wv = (2 * hh, 2 * ww) if upsample2x else (hh, ww)
    ho = (hv + pt + pb - ks) // stride + 1
    wo = (wv + pl + pr - ks) // stride + 1
    if cin <= 8 or (cin == 9 and cout % 8 == 0) or (cout <= 8 and (cin % 8 != 0 or cin < 64)):  # 9: the inpainting UNet's conv_in
        if x_lo is not None:
            raise L.CrgError("conv2d: thin-channel convs take the fp32 tensor, not split planes")
        if stride != 1 or upsample2x or x2 is not None or cvec is not None or residual is not None or gn is not None or (pt, pl, pb, pr) != (ks // 2,) * 4:
            raise L.CrgError("conv2d: thin-channel convs support only stride 1, 'same' padding, no fusions (no fused GroupNorm either)")
        y = empty_image(n, cout, ho, wo, x.dtype, x.device)
        _call("crg_conv_small", x, _p(x), _p(f32_vec(weight)), _p(f32_vec(bias)), _p(y), n, hh, ww, cin, cout, ks, _act_dt(x), _act_dt(y))
        return y
    planes = x_lo is not None
    split = planes or x.dtype == torch.float32
    up2 = bool(upsample2x) and (planes if subpixel is None else subpixel) and stride == 1 and (pt, pl, pb, pr) == (1, 1, 1, 1) and x2 is None and cvec is None and residual is None \
        and gn is None and upsample_subpixel_ok(x, weight, x_lo)
    hi, lo = packed_weight(weight, L.PACK_CONV_UP2 if up2 else L.PACK_CONV, split)
    y = empty_image(n, cout, ho, wo, torch.float32 if planes else x.dtype, x.device)
    if residual is not None:
        residual = to_channels_last(residual)
        if residual.shape != y.shape or residual.dtype != y.dtype:
            raise L.CrgError("conv2d: residual must match the output in shape and dtype")
    if cvec is not None:
        if cvec.dtype != torch.float32 or tuple(cvec.shape) != (n, cout) or cvec.stride(1) != 1 or cvec.stride(0) % 4:
            raise L.CrgError("conv2d: cvec must be fp32 [N, Cout] with unit column stride and 16-byte aligned rows")
        if n > 1 and cvec.stride(0) < cout:  # one row expanded over the batch (stride 0): the C ABI reads a row stride of 0 as "Cout"
            cvec = cvec.contiguous()
    a = L.ConvArgs(x=x.data_ptr(), x2=x2.data_ptr() if x2 is not None else None, C1=c1, C2=c2, w=hi.data_ptr(),
                   w_lo=lo.data_ptr() if lo is not None else None, bias=_p(f32_vec(bias)).value, cvec=_p(cvec).value,
                   cvec_ld=cvec.stride(0) if cvec is not None else 0, residual=_p(residual).value, y=y.data_ptr(), N=n, H=hh, W=ww, Cout=cout, Ho=ho, Wo=wo, ksize=ks, stride=stride,
                   pad_t=pt, pad_l=pl, upsample2x=2 if up2 else int(upsample2x), x_dtype=_act_dt(x), y_dtype=_act_dt(y),
                   prec=L.PREC_BF16X3 if planes else _prec(x), x_lo=x_lo.data_ptr() if planes else None)
    y_norm = keep = None
    if gn is not None:
        gw, gb, groups, eps, silu = gn
        if planes or y.dtype != HALF or cout % groups or (cout // groups) % 8:
            raise L.CrgError("conv2d: the fused GroupNorm takes bf16 outputs with 8-aligned groups")
        y_norm = empty_image(n, cout, ho, wo, y.dtype, x.device)
        keep = (f32_vec(gw), f32_vec(gb))
        a.gn_gamma, a.gn_beta, a.gn_y = keep[0].data_ptr(), keep[1].data_ptr(), y_norm.data_ptr()
        a.gn_groups, a.gn_silu, a.gn_eps = int(groups), int(bool(silu)), float(eps)
    stats = _gn_stats_buffer(n * ho * wo, cout, ho * wo, x.dtype, y.dtype, x.device) if (gn_stats and gn is None and (planes or x.dtype == HALF)) else None
    if stats is not None and planes and (cout % 4 or knobs.VAE_GN_STATS is False):
        stats = None
    rows = C.c_int(32)
    if stats is not None:
        a.gn_stats = stats.data_ptr()
        if knobs.GN_TILE and not planes:
            a.gn_stats_rows = C.pointer(rows)  # the launch reports the granularity it wrote
    _call("crg_conv2d", x, C.byref(a))
    if stats is not None:
        y._crg_gn = (stats, y._version, ho * wo, rows.value)
    return y if gn is None else (y, y_norm)


def _conv2d_mx(x16, x8, weight, bias, stride, padding, upsample2x, x2, cvec, residual, x_lo, gn_stats, gn):
    x16 = to_channels_last(x16)
    n, c, hh, ww = x16.shape
    cout, cin, ks, _ = weight.shape
    if x16.dtype != torch.float16 or x8.dtype != torch.uint8 or tuple(x8.shape) != (n, hh, ww, 2 * c) or not x8.is_contiguous():
        raise L.CrgError("conv2d(x_mx=): x must be the fp16 plane [N, C, H, W] (channels-last) and x_mx the uint8 plane [N, H, W, 2 C]")
    if ks != 3 or stride != 1 or padding not in (1, (1, 1, 1, 1)) or upsample2x or x2 is not None or x_lo is not None or gn is not None or cvec is not None \
            or cin != c or c % 64:
        raise L.CrgError("conv2d(x_mx=): 3x3 / stride 1 / pad 1 convs with Cin % 64 == 0 only (no upsample / concat / fused GroupNorm)")
    w16, w8, whi, wlo = packed_weight_mx(weight)
    y = empty_image(n, cout, hh, ww, torch.float32, x16.device)
    if residual is not None:
        residual = to_channels_last(residual)
        if residual.shape != y.shape or residual.dtype != y.dtype:
            raise L.CrgError("conv2d: residual must match the output in shape and dtype")
    a = L.ConvArgs(x=x16.data_ptr(), x2=None, C1=c, C2=0, w=w16.data_ptr(), w_lo=w8.data_ptr(), bias=_p(f32_vec(bias)).value, cvec=None, cvec_ld=0,
                   residual=_p(residual).value, y=y.data_ptr(), N=n, H=hh, W=ww, Cout=cout, Ho=hh, Wo=ww, ksize=3, stride=1, pad_t=1, pad_l=1,
                   upsample2x=0, x_dtype=L.BF16, y_dtype=L.F32, prec=L.PREC_F16MX, x_lo=x8.data_ptr())
    a.mx_log2[0], a.mx_log2[1], a.mx_log2[2], a.mx_log2[3] = whi, wlo, MX_X_LOG2[0], MX_X_LOG2[1]
    stats = _gn_stats_buffer(n * hh * ww, cout, hh * ww, HALF, torch.float32, x16.device) if (gn_stats and knobs.VAE_GN_STATS and cout % 4 == 0) else None
    if stats is not None:
        a.gn_stats = stats.data_ptr()
    _call("crg_conv2d", x16, C.byref(a))
    if stats is not None:
        y._crg_gn = (stats, y._version, hh * ww)
    return y


def upsample_subpixel_ok(x: torch.Tensor, weight: torch.Tensor, x_lo: Optional[torch.Tensor] = None) -> bool:
    """Can conv2d(x, weight, upsample2x=True[, x_lo=x_lo]) (3x3, stride 1, pad 1, no fusions; 16-bit x: subpixel=True) run in the sub-pixel form - four 2x2 convs
    on the source grid with pre-summed weights (crg_conv_args.upsample2x = 2)?  Mirrors the native conditions: a 16-bit x plane (half-type
    activations, or the hi / lo planes of an fp32 one), Cin % 64 == 0, Cout > 32, H * W a multiple of the 128-pixel tile and a source width
    the row-halo kernel's buffers take (16..128 dividing 128, or a multiple of 128).  Everything else keeps the gather form."""
    if not (knobs.UP_SUBPIX and x.is_cuda and x.dim() == 4 and weight.dim() == 4 and tuple(weight.shape[2:]) == (3, 3)):
        return False
    if x.dtype != HALF or (x_lo is not None and (x_lo.dtype != HALF or x_lo.shape != x.shape)):
        return False
    n, c, hh, ww = x.shape
    if weight.shape[1] != c or c % 64 or weight.shape[0] <= 32:
        return False
    return (hh * ww) % 128 == 0 and ww >= 16 and (128 % ww == 0 if ww <= 128 else ww % 128 == 0)


def mx_conv_ok(x: torch.Tensor, conv_weight: torch.Tensor) -> bool:
    """Would conv2d(x16, w, x_mx=...) take this fp32 activation / 3x3 weight pair (and is the MX form enabled)?"""
    return (knobs.VAE_MX and x.is_cuda and x.dtype == torch.float32 and conv_weight.dim() == 4 and conv_weight.shape[2] == 3 and x.shape[1] % 64 == 0
            and conv_weight.shape[1] == x.shape[1] and conv_weight.shape[0] > 8 and conv_weight.shape[0] % 4 == 0)


def conv1x1(x: torch.Tensor, weight: torch.Tensor, bias=None, residual: Optional[torch.Tensor] = None, gn_stats: bool = False) -> torch.Tensor:
    """1x1 conv on a channels-last image == linear over its token view (no copy either way)."""
    x = to_channels_last(x)
    n, c, hh, ww = x.shape
    res_t = tokens_of(to_channels_last(residual)) if residual is not None else None
    y = linear(tokens_of(x), weight, bias, residual=res_t, gn_hw=hh * ww if gn_stats else None)
    return image_of_stats(y, hh, ww)
