"""FILM frame interpolation (film.hip).

Images are [N, C, H, W] with channels-last strides, or a CHANNEL SLICE of such a tensor: rows of C consecutive channels, `ld` elements
apart.  Every op takes its destination(s) as such a slice (`out=buffer[:, off:off + C]`), which is how the reference's torch.cat's
become writes; without `out` a dense channels-last tensor is allocated.  fp32 only.
"""
import ctypes as C
from typing import Optional, Tuple

import torch

from .. import _lib as L
from ._base import HALF, _call, _need_cuda, _p, _written, empty_image


def _film_rows(t: torch.Tensor, what: str, dtype=torch.float32) -> Tuple[int, int, int, int, int]:
    """(N, C, H, W, ld) of a channels-last image or of a channel slice of one"""
    if t.dim() != 4 or t.dtype != dtype:
        raise L.CrgError(f"{what}: a 4-D {dtype} image expected, got {tuple(t.shape)} {t.dtype}")
    n, c, hh, ww = t.shape
    sn, sc, sh, sw = t.stride()
    ld = sw if ww > 1 else (sh // ww if hh > 1 else (sn // (hh * ww) if n > 1 else c))
    ok = (c == 1 or sc == 1) and ld >= c and (ww == 1 or sw == ld) and (hh == 1 or sh == ww * ld) and (n == 1 or sn == hh * ww * ld)
    if not ok or min(n, c, hh, ww) < 1:
        raise L.CrgError(f"{what}: a channels-last image or a channel slice of one expected, got shape {tuple(t.shape)} strides {t.stride()}")
    return n, c, hh, ww, ld


def _film_dst(out, n, c, hh, ww, device, what, dtype=torch.float32):
    if out is None:
        out = empty_image(n, c, hh, ww, dtype, device)
    _need_cuda(out)
    got = _film_rows(out, what, dtype)
    if got[:4] != (n, c, hh, ww):
        raise L.CrgError(f"{what}: destination {tuple(out.shape)} does not match [{n}, {c}, {hh}, {ww}]")
    return out, got[4]


def _film_planes(planes, n, c, hh, ww, device, what):
    """None / False -> no planes; True -> fresh dense planes; (hi, lo) -> two half-type destinations of one row stride"""
    if planes is None or planes is False:
        return None, None, 0
    hi, lo = (None, None) if planes is True else planes
    hi, ldh = _film_dst(hi, n, c, hh, ww, device, what + " (hi plane)", HALF)
    lo, ldl = _film_dst(lo, n, c, hh, ww, device, what + " (lo plane)", HALF)
    if ldh != ldl:
        raise L.CrgError(f"{what}: the two planes must share one row stride ({ldh} / {ldl})")
    return hi, lo, ldh


def _film_scale(scale: Optional[torch.Tensor], n: int, what: str) -> Optional[torch.Tensor]:
    """The per-sample factors as contiguous fp32 [N], or None"""
    if scale is None:
        return None
    if scale.dtype != torch.float32 or scale.numel() != n:
        raise L.CrgError(f"{what}: scale must hold {n} fp32 values")
    return scale.reshape(n).contiguous()


def warp_flow(src: torch.Tensor, flow: torch.Tensor, scale: Optional[torch.Tensor] = None, *, out: Optional[torch.Tensor] = None, planes=None, fp32: bool = True):
    """util.warp(src, scale * flow) of the FILM interpolator: out[n, :, y, x] = bilinear lookup of src[n] at (x + s flow[n, 0, y, x],
    y + s flow[n, 1, y, x]), the position clamped to the image; s = scale[n] (fp32 [N]) or 1.  src [N, C, H, W], flow [N, 2, H, W]: fp32
    channels-last images or channel slices.  Returns out, or (out, (hi, lo)) with `planes`; `fp32=False` writes the planes alone."""
    _need_cuda(src, flow, scale, out)
    n, c, hh, ww, lds = _film_rows(src, "warp_flow: src")
    ldf = _film_rows(flow, "warp_flow: flow")[4]
    if tuple(flow.shape) != (n, 2, hh, ww):
        raise L.CrgError(f"warp_flow: flow {tuple(flow.shape)} does not match src {tuple(src.shape)}")
    scale = _film_scale(scale, n, "warp_flow")
    ldd = 0
    if fp32:
        out, ldd = _film_dst(out, n, c, hh, ww, src.device, "warp_flow: out")
    elif out is not None or not planes:
        raise L.CrgError("warp_flow: fp32=False writes planes only")
    hi, lo, ldp = _film_planes(planes, n, c, hh, ww, src.device, "warp_flow")
    a = L.FilmWarpArgs(src=src.data_ptr(), ld_src=lds, flow=flow.data_ptr(), ld_flow=ldf, scale=_p(scale).value, dst=_p(out).value, ld_dst=ldd,
                       hi=_p(hi).value, lo=_p(lo).value, ld_planes=ldp, N=n, H=hh, W=ww, C=c)
    _call("crg_film_warp", src, C.byref(a))
    for t in (out, hi, lo):
        if t is not None:
            _written(t)
    return out if hi is None else (out, (hi, lo))


def avg_pool2(x: torch.Tensor, *, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """F.avg_pool2d(x, 2, 2) of an fp32 channels-last image or channel slice; odd sizes floor."""
    _need_cuda(x, out)
    n, c, hh, ww, lds = _film_rows(x, "avg_pool2: x")
    if hh < 2 or ww < 2:
        raise L.CrgError(f"avg_pool2: a {hh} x {ww} image has no 2 x 2 window")
    out, ldd = _film_dst(out, n, c, hh // 2, ww // 2, x.device, "avg_pool2: out")
    _call("crg_film_pool2", x, _p(x), lds, _p(out), ldd, n, hh, ww, c)
    return _written(out)


def flow_up2_add(v: torch.Tensor, residual: Optional[torch.Tensor] = None, *, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """residual + F.interpolate(2 * v, size=(2 h, 2 w), mode='bilinear') of a flow v [N, 2, h, w]; without residual the upsampled flow."""
    _need_cuda(v, residual, out)
    n, c, hh, ww, ldv = _film_rows(v, "flow_up2_add: v")
    if c != 2:
        raise L.CrgError(f"flow_up2_add: a flow has 2 channels, got {c}")
    ldr = 0
    if residual is not None:
        ldr = _film_rows(residual, "flow_up2_add: residual")[4]
        if tuple(residual.shape) != (n, 2, 2 * hh, 2 * ww):
            raise L.CrgError(f"flow_up2_add: residual {tuple(residual.shape)} is not twice the size of {tuple(v.shape)}")
    out, ldd = _film_dst(out, n, 2, 2 * hh, 2 * ww, v.device, "flow_up2_add: out")
    _call("crg_film_flow_up", v, _p(v), ldv, _p(residual), ldr, _p(out), ldd, n, hh, ww)
    return _written(out)


def leaky_split(x: torch.Tensor, slope: float = 0.2, *, out: Optional[torch.Tensor] = None, fp32: bool = True, planes=None, pool=None,
                scale: Optional[torch.Tensor] = None):
    """LeakyReLU(slope) of a conv's fp32 output x in one pass, as any of: the fp32 image (`out`, a slice or - None - a fresh tensor; x itself
    is allowed; `fp32=False`: not written), the (hi, lo) half-type planes of the fp32-class conv (`planes`: True or two destinations) and
    its 2 x 2 mean (`pool`: True or a destination; floor).  `scale` fp32 [N]: every value of sample n is multiplied by scale[n] after the
    activation.  Returns (y, planes, pooled) with None for what was not asked for."""
    _need_cuda(x, out, scale)
    n, c, hh, ww, ldx = _film_rows(x, "leaky_split: x")
    scale = _film_scale(scale, n, "leaky_split")
    y, ldy = (None, 0)
    if fp32:
        y, ldy = _film_dst(out, n, c, hh, ww, x.device, "leaky_split: out")
    elif out is not None:
        raise L.CrgError("leaky_split: fp32=False takes no `out`")
    hi, lo, ldp = _film_planes(planes, n, c, hh, ww, x.device, "leaky_split")
    pl, ldq = (None, 0)
    if pool is not None and pool is not False:
        if hh < 2 or ww < 2:
            raise L.CrgError(f"leaky_split: a {hh} x {ww} image has no 2 x 2 window")
        pl, ldq = _film_dst(None if pool is True else pool, n, c, hh // 2, ww // 2, x.device, "leaky_split: pool")
    if y is None and hi is None and pl is None:
        raise L.CrgError("leaky_split: nothing to write")
    a = L.FilmActArgs(x=x.data_ptr(), ld_x=ldx, y=_p(y).value, ld_y=ldy, hi=_p(hi).value, lo=_p(lo).value, ld_planes=ldp, pool=_p(pl).value, ld_pool=ldq,
                      scale=_p(scale).value, N=n, H=hh, W=ww, C=c, slope=float(slope))
    _call("crg_film_act", x, C.byref(a))
    for t in (y, hi, lo, pl):
        if t is not None:
            _written(t)
    return y, (None if hi is None else (hi, lo)), pl


def scale_into(x: torch.Tensor, scale: Optional[torch.Tensor] = None, *, out: torch.Tensor) -> torch.Tensor:
    """out = scale[n] * x (scale None: a copy) into a channel slice: the same kernel with slope 1, which is the identity."""
    return leaky_split(x, 1.0, out=out, scale=scale)[0]
