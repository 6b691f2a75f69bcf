"""Temporal layers of the video UNet and the VideoDecoder (video.hip, video_x3.hip).

Tokens are [F, S, C] contiguous with F = b * T frames (video-major) of S pixels: the bytes of the [(b t), C, h, w] channels-last
image the spatial layers work on, so `tokens_of` / `image_of` move between the two for free and no (b t) s c <-> (b s) t c rearrange
ever runs.
"""
import ctypes as C
from typing import Optional, Tuple

import torch

from .. import _lib as L
from ._base import HALF, _act_dt, _call, _need_cuda, _p, _pack_cache, _written, f32_vec
from .gemm import linear
from .packing import packed_weight
from .steps import axpby_

MAX_FRAMES = 32  # crg_attention_frames


def _frame_tokens(x: torch.Tensor, frames: int, what: str) -> Tuple[int, int, int, int]:
    if x.dim() != 3 or not x.is_contiguous():
        raise L.CrgError(f"{what}: contiguous [frames, pixels, channels] tokens expected, got shape {tuple(x.shape)} with strides {x.stride()}")
    F, S, Cc = x.shape
    if frames < 1 or F < 1 or S < 1 or F % frames:
        raise L.CrgError(f"{what}: {F} frames of {S} pixels do not split into videos of {frames} frames")
    return F // frames, F, S, Cc


def frames_weight(w: torch.Tensor) -> torch.Tensor:
    """[Cout, Cin, 3, 1, 1] (or [Cout, Cin, 3]) -> the [Cout, 3 * Cin] matrix crg_conv_frames multiplies by: tap-major, channel-minor.
    Cached on the identity + version of `w` like every packed weight; the result then goes through `packed_weight` (LINEAR)."""
    if w.dim() not in (3, 5) or w[0, 0].numel() != 3 or w.shape[2] != 3:
        raise L.CrgError(f"conv_frames: a [Cout, Cin, 3, 1, 1] weight expected, got {tuple(w.shape)}")
    r = _pack_cache.get((w,), ("frames",))
    if r is None:
        r = _pack_cache.put((w,), ("frames",), w.detach().reshape(w.shape[0], w.shape[1], 3).permute(0, 2, 1).reshape(w.shape[0], -1).contiguous())
    return r


def _frames_taps(w: torch.Tensor):
    """The three [Cout, Cin] tap matrices W_-1, W_0, W_+1 of a frame conv weight (the composed fp32-class route), cached like frames_weight."""
    r = _pack_cache.get((w,), ("frame_taps",))
    if r is None:
        w3 = w.detach().reshape(w.shape[0], w.shape[1], 3)
        r = _pack_cache.put((w,), ("frame_taps",), tuple(w3[:, :, d].contiguous() for d in range(3)))
    return r


def _frame_vec(v: Optional[torch.Tensor], F: int, what: str) -> Optional[torch.Tensor]:
    if v is None:
        return None
    if v.numel() != F:
        raise L.CrgError(f"{what}: one value per frame ({F}) expected, got shape {tuple(v.shape)}")
    return v.detach().reshape(F).float().contiguous()


def _frame_conv_widths(what: str, weight: torch.Tensor, Cin: int, residual, rscale) -> int:
    """Cout of a frame conv whose weight takes Cin channels (both multiples of 32; rscale only with a residual)"""
    Cout = weight.shape[0]
    if weight.shape[1] != Cin:
        raise L.CrgError(f"{what}: weight {tuple(weight.shape)} does not match {Cin} input channels")
    if Cin % 32 or Cout % 32:
        raise L.CrgError(f"{what}: Cin={Cin} / Cout={Cout} must be multiples of 32")
    if rscale is not None and residual is None:
        raise L.CrgError(f"{what}: rscale needs a residual")
    return Cout


def _frame_conv_vectors(what: str, cvec, rscale, F: int, Cout: int):
    """(cvec as fp32 [F, Cout], rscale as fp32 [F]), each None when not given"""
    if cvec is not None:
        if cvec.numel() != F * Cout:
            raise L.CrgError(f"{what}: cvec must hold [{F}, {Cout}] values, got {tuple(cvec.shape)}")
        cvec = cvec.detach().reshape(F, Cout).float().contiguous()
    return cvec, _frame_vec(rscale, F, f"{what}: rscale")


def conv_frames(x: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor] = None, *, frames: int, cvec: Optional[torch.Tensor] = None,
                residual: Optional[torch.Tensor] = None, rscale: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The (3, 1, 1) conv along the frame axis of x [b * frames, S, Cin] tokens, zero padding at both ends of every video:
    y[v, t] = sum_d W_d x[v, t + d] + bias + cvec[v * frames + t], then y = residual + rscale[v * frames + t] * y when a residual is given
    (rscale None = 1).  cvec: [b * frames, Cout], rscale: b * frames values, residual: like y.  A frame outside its video contributes zero
    by selection - its memory is never read.  Half type: one launch of crg_conv_frames.  fp32: composed from the fp32-class ops, per
    video three row-shifted `linear` calls summed in fp32 (the video UNet runs in the half type; the fp32-class video VAE holds
    pre-split planes and calls `conv_frames_x3`, one launch)."""
    _need_cuda(x, weight, bias, cvec, residual, rscale)
    b, F, S, Cin = _frame_tokens(x, frames, "conv_frames")
    Cout = _frame_conv_widths("conv_frames", weight, Cin, residual, rscale)
    if residual is not None and (residual.shape != (F, S, Cout) or residual.dtype != x.dtype or not residual.is_contiguous()):
        raise L.CrgError("conv_frames: the residual must be contiguous and match the output in shape and dtype")
    cvec, rs = _frame_conv_vectors("conv_frames", cvec, rscale, F, Cout)
    _act_dt(x)
    if x.dtype == torch.float32:
        w0, w1, w2 = _frames_taps(weight)
        y = torch.empty((F, S, Cout), dtype=torch.float32, device=x.device)
        for v in range(b):
            xv, yv = x[v * frames:(v + 1) * frames], y[v * frames:(v + 1) * frames]
            yv.copy_(linear(xv, w1, bias))
            if frames > 1:
                axpby_(yv[1:], linear(xv[:-1], w0), 1.0, 1.0)
                axpby_(yv[:-1], linear(xv[1:], w2), 1.0, 1.0)
        if cvec is not None:
            y = add_frames(y, cvec)
        if residual is not None:
            y = lincomb_frames(None, residual, rs, y)
        return y
    hi, _ = packed_weight(frames_weight(weight), L.PACK_LINEAR, False)
    bb = f32_vec(bias)
    y = torch.empty((F, S, Cout), dtype=x.dtype, device=x.device)
    a = L.ConvFramesArgs(x=x.data_ptr(), w=hi.data_ptr(), bias=_p(bb).value, cvec=_p(cvec).value, cvec_ld=Cout, residual=_p(residual).value,
                         rscale=_p(rs).value, y=y.data_ptr(), b=b, T=frames, S=S, Cin=Cin, Cout=Cout)
    _call("crg_conv_frames", x, C.byref(a))
    return y


def conv_frames_x3(x_hi: torch.Tensor, x_lo: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor] = None, *, frames: int,
                   cvec: Optional[torch.Tensor] = None, residual: Optional[torch.Tensor] = None, rscale: Optional[torch.Tensor] = None,
                   out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """`conv_frames` in the fp32 class, one launch of crg_conv_frames_x3: x_hi, x_lo are the two half-type planes [b * frames, S, Cin] of an
    fp32 activation (group_norm(split=True) / split_bf16, as tokens), the weight's planes come from the pack cache, residual and result
    are fp32 [b * frames, S, Cout].  `out`: write there instead of a new tensor (it may be the residual itself)."""
    _need_cuda(x_hi, x_lo, weight, bias, cvec, residual, rscale, out)
    if x_hi.dtype != HALF or x_lo.dtype != HALF or x_hi.shape != x_lo.shape or not x_lo.is_contiguous():
        raise L.CrgError(f"conv_frames_x3: x_hi / x_lo must be two contiguous half-type planes of one shape, got {tuple(x_hi.shape)} {x_hi.dtype} "
                         f"and {tuple(x_lo.shape)} {x_lo.dtype}")
    b, F, S, Cin = _frame_tokens(x_hi, frames, "conv_frames_x3")
    Cout = _frame_conv_widths("conv_frames_x3", weight, Cin, residual, rscale)
    for t, what in ((residual, "residual"), (out, "out")):
        if t is not None and (t.shape != (F, S, Cout) or t.dtype != torch.float32 or not t.is_contiguous()):
            raise L.CrgError(f"conv_frames_x3: {what} must be contiguous fp32 [{F}, {S}, {Cout}]")
    cvec, rs = _frame_conv_vectors("conv_frames_x3", cvec, rscale, F, Cout)
    hi, lo = packed_weight(frames_weight(weight), L.PACK_LINEAR, True)
    bb = f32_vec(bias)
    y = out if out is not None else torch.empty((F, S, Cout), dtype=torch.float32, device=x_hi.device)
    a = L.ConvFramesX3Args(x_hi=x_hi.data_ptr(), x_lo=x_lo.data_ptr(), w_hi=hi.data_ptr(), w_lo=lo.data_ptr(), bias=_p(bb).value, cvec=_p(cvec).value,
                           cvec_ld=Cout, residual=_p(residual).value, rscale=_p(rs).value, y=y.data_ptr(), b=b, T=frames, S=S, Cin=Cin, Cout=Cout)
    _call("crg_conv_frames_x3", x_hi, C.byref(a))
    return _written(y) if out is not None else y


def conv_frames_thin(x: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor] = None, *, frames: int) -> torch.Tensor:
    """The (3, 1, 1) frame conv on C <= 8 channels (AE3DConv.time_mix_conv): x [b * frames, S, C] tokens, half type or fp32; weight
    [C, C, 3, 1, 1] and bias are taken in fp32.  fp32 FMAs in a fixed order, one rounding to x.dtype; frames outside a video are not read."""
    _need_cuda(x, weight, bias)
    b, F, S, Cc = _frame_tokens(x, frames, "conv_frames_thin")
    if not 1 <= Cc <= 8:
        raise L.CrgError(f"conv_frames_thin: {Cc} channels (1 .. 8; wider convs are conv_frames)")
    if weight.dim() not in (3, 5) or weight.shape[0] != Cc or weight.shape[1] != Cc or weight[0, 0].numel() != 3:
        raise L.CrgError(f"conv_frames_thin: a [{Cc}, {Cc}, 3, 1, 1] weight expected, got {tuple(weight.shape)}")
    if bias is not None and bias.numel() != Cc:
        raise L.CrgError(f"conv_frames_thin: {bias.numel()} bias values for {Cc} channels")
    y = torch.empty_like(x)
    _call("crg_conv_frames_thin", x, _p(x), _p(f32_vec(weight)), _p(f32_vec(bias)), _p(y), b, frames, S, Cc, _act_dt(x))
    return y


def attention_frames(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, heads: int, *, frames: int, scale: Optional[float] = None) -> torch.Tensor:
    """Self-attention across the frames of every pixel: for each (video, pixel, head) softmax(q k^T * scale) v over the `frames` <= 32
    frames.  q, k, v: [b * frames, S, C] tokens of one dtype (half type or fp32); each may be a column slice of one fused projection
    output - rows keep the parent's stride, nothing is copied.  Returns [b * frames, S, C] contiguous.  scale: d_head ** -0.5 by default."""
    _need_cuda(q, k, v)
    if q.dim() != 3 or q.shape != k.shape or q.shape != v.shape or q.dtype != k.dtype or q.dtype != v.dtype:
        raise L.CrgError("attention_frames: q, k, v of one [frames, pixels, channels] shape and dtype expected")
    F, S, Cc = q.shape
    if frames < 1 or F % frames:
        raise L.CrgError(f"attention_frames: {F} frames do not split into videos of {frames}")
    if Cc % heads:
        raise L.CrgError(f"attention_frames: {Cc} channels do not split into {heads} heads")
    Dh = Cc // heads
    align = 16 // q.element_size()

    def rows(t):  # [F, S, C] as [F * S] rows one stride apart, 16-byte aligned
        if t.stride(2) != 1 or t.stride(0) != S * t.stride(1) or t.stride(1) % align or t.stride(1) < Cc or t.data_ptr() % 16:
            t = t.contiguous()
        return t, t.stride(1)
    q, ldq = rows(q)
    k, ldk = rows(k)
    v, ldv = rows(v)
    o = torch.empty((F, S, Cc), dtype=q.dtype, device=q.device)
    a = L.AttnFramesArgs(q=q.data_ptr(), ldq=ldq, k=k.data_ptr(), ldk=ldk, v=v.data_ptr(), ldv=ldv, o=o.data_ptr(), ldo=Cc,
                         b=F // frames, T=frames, S=S, H=heads, Dh=Dh, scale=float(scale if scale is not None else Dh ** -0.5), dtype=_act_dt(q))
    _call("crg_attention_frames", q, C.byref(a))
    return o


def add_frames(x: torch.Tensor, emb: torch.Tensor) -> torch.Tensor:
    """x [F, S, C] tokens + emb [F, C]: one channel vector per frame added to all of its pixels (dtype of x; C % 8 == 0)."""
    _need_cuda(x, emb)
    if x.dim() != 3 or not x.is_contiguous() or emb.numel() != x.shape[0] * x.shape[2]:
        raise L.CrgError(f"add_frames: contiguous [F, S, C] tokens and [F, C] vectors expected, got {tuple(x.shape)} and {tuple(emb.shape)}")
    F, S, Cc = x.shape
    emb = emb.detach().reshape(F, Cc).to(x.dtype).contiguous()
    y = torch.empty_like(x)
    _call("crg_add_frames", x, _p(x), _p(emb), _p(y), F, S, Cc, _act_dt(x))
    return y


def lincomb_frames(a: Optional[torch.Tensor], x: torch.Tensor, c: Optional[torch.Tensor], z: torch.Tensor) -> torch.Tensor:
    """a[f] * x[f] + c[f] * z[f] with one coefficient per leading index f (None = 1, exactly).  x, z: dense, same shape / strides / dtype.
    fp32 arithmetic with each product and the sum rounded on its own - on fp32 tensors the bits of the framework's a * x + c * z."""
    _need_cuda(a, x, c, z)
    if x.shape != z.shape or x.stride() != z.stride() or x.dtype != z.dtype or not x.is_contiguous():
        raise L.CrgError("lincomb_frames: contiguous operands of one shape and dtype expected")
    F = x.shape[0]
    per = x.numel() // max(F, 1)
    av, cv = _frame_vec(a, F, "lincomb_frames: a"), _frame_vec(c, F, "lincomb_frames: c")
    y = torch.empty_like(x)
    _call("crg_lincomb_frames", x, _p(av), _p(x), _p(cv), _p(z), _p(y), F, per, _act_dt(x))
    return y


def blend_frames(alpha: torch.Tensor, x: torch.Tensor, z: torch.Tensor) -> torch.Tensor:
    """The per-frame AlphaBlender: alpha[f] * x + (1 - alpha[f]) * z (axpby_ only takes scalars; a mixed image_only_indicator under
    `learned_with_images` needs one alpha per frame).  alpha: one fp32 value per leading index of x."""
    al = _frame_vec(alpha, x.shape[0], "blend_frames: alpha")
    return lincomb_frames(al, x, 1.0 - al, z)
