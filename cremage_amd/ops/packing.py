"""Packed images of weights (cached on the identity and version of their sources) and the MX planes of activations."""
import math
from typing import Optional, Tuple

import torch

from .. import _lib as L
from ._base import _DT, HALF, _call, _dt, _need_cuda, _p, _pack_cache, to_channels_last


def _pack_source(w: torch.Tensor) -> torch.Tensor:
    """The detached, contiguous weight in a dtype crg_pack_* reads"""
    src = w.detach().contiguous()
    return src if src.dtype in _DT else src.float()  # e.g. bfloat16 parameters handed to the fp16-operand build


def packed_weight(w: torch.Tensor, kind: int, split: bool) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
    """bf16 [N, K] image of a Linear / conv weight (+ bf16 residual plane when `split`)."""
    _need_cuda(w)
    if kind == L.PACK_LINEAR and not split and w.dtype == HALF and w.is_contiguous():
        return w.detach().reshape(w.shape[0], -1), None  # zero-copy: already the packed image
    r = _pack_cache.get((w,), (kind, split))
    if r is not None:
        return r
    src = _pack_source(w)
    rows = n_out = src.shape[0]
    if kind == L.PACK_CONV:
        n_in, ks = src.shape[1], src.shape[2]
        cols = n_in * ks * ks
    elif kind == L.PACK_CONV_UP2:  # the four parity slabs [Cout][4 Cin] of the sub-pixel upsample conv, one after the other
        n_in, ks = src.shape[1], src.shape[2]
        rows, cols = 4 * n_out, 4 * n_in
    else:
        n_in, ks = src[0].numel(), 1
        cols = n_in
    hi = torch.empty((rows, cols), dtype=HALF, device=w.device)
    lo = torch.empty_like(hi) if split else None
    _call("crg_pack_weight", w, _p(src), _dt(src), kind, n_out, n_in, ks, _p(hi), _p(lo))
    return _pack_cache.put((w,), (kind, split), (hi, lo))


def packed_ln_weight(w: torch.Tensor, gamma: torch.Tensor, beta: torch.Tensor, bias: Optional[torch.Tensor], geglu: bool):
    """(W o gamma in the library's half type [N, K], column sums of that rounded image fp32 [N], folded bias W beta + b fp32 [N]) -
    crg_pack_ln_weight; cached on the identity + version of all four sources (LoRA-merged weights arrive as their own tensors)."""
    _need_cuda(w, gamma, beta, bias)
    srcs = (w, gamma, beta) + ((bias,) if bias is not None else ())
    r = _pack_cache.get(srcs, ("ln", geglu, bias is not None))
    if r is not None:
        return r
    src = _pack_source(w.detach().reshape(w.shape[0], -1))
    n_out, n_in = src.shape
    dw = torch.empty((n_out, n_in), dtype=HALF, device=w.device)
    ds = torch.empty((n_out,), dtype=torch.float32, device=w.device)
    db = torch.empty((n_out,), dtype=torch.float32, device=w.device)
    g32, b32 = gamma.detach().float().contiguous(), beta.detach().float().contiguous()
    bb = bias.detach().float().contiguous() if bias is not None else None
    _call("crg_pack_ln_weight", w, _p(src), _dt(src), _p(g32), _p(b32), _p(bb), L.PACK_GEGLU if geglu else L.PACK_LINEAR, n_out, n_in, _p(dw), _p(ds), _p(db))
    return _pack_cache.put(srcs, ("ln", geglu, bias is not None), (dw, ds, db))


def packed_geglu_bias(b: torch.Tensor) -> torch.Tensor:
    r = _pack_cache.get((b,), ("geglu_bias",))
    if r is None:
        src = b.detach().float().contiguous()
        r = torch.empty_like(src)
        _call("crg_pack_geglu_bias", b, _p(src), src.numel(), _p(r))
        _pack_cache.put((b,), ("geglu_bias",), r)
    return r


# ---------------------------------------------------------------------------------- MX planes (CRG_PREC_F16MX)
# The fp32-class 3x3 conv in two matrix passes' worth of cycles instead of three: operands as a fp16 plane plus a plane of e4m3 pairs
# (include/crg_hip.h, crg_split_mx).  Activations behind GroupNorm + SiLU are O(1): fixed power-of-two scales (hi8: x * 2^4, saturating at
# |x| = 28 - the cross terms lose precision there, nothing else; lo8: (x - half(x)) * 2^15).  Weights: scales from the tensor's maximum at
# pack time.  The VAE uses it only under knobs.VAE_MX.
MX_X_LOG2 = (4, 15)


def packed_weight_mx(w: torch.Tensor):
    """(w16 fp16 [Cout, 9 Cin], w8 uint8 [Cout, 9 Cin / 64, 128], hi_log2, lo_log2) of a 3x3 conv weight (crg_pack_weight_mx)."""
    _need_cuda(w)
    r = _pack_cache.get((w,), ("mx",))
    if r is not None:
        return r
    src = _pack_source(w)
    n_out, n_in = src.shape[0], src.shape[1]
    amax = float(src.detach().abs().max().item())  # pack time only (outside graph capture: the warm-up calls pack)
    hi = int(math.floor(math.log2(448.0 / max(amax, 1e-30)))) if amax > 0 else 0
    hi = max(-60, min(60, hi))
    lo = hi + 11
    w16 = torch.empty((n_out, 9 * n_in), dtype=torch.float16, device=w.device)
    w8 = torch.empty((n_out, 9 * n_in // 64, 128), dtype=torch.uint8, device=w.device)
    _call("crg_pack_weight_mx", w, _p(src), _dt(src), n_out, n_in, _p(w16), _p(w8), hi, lo)
    return _pack_cache.put((w,), ("mx",), (w16, w8, hi, lo))


def _empty_mx(n, c, hh, ww, device):
    x16 = torch.empty((n, hh, ww, c), dtype=torch.float16, device=device).permute(0, 3, 1, 2)
    x8 = torch.empty((n, hh, ww, 2 * c), dtype=torch.uint8, device=device)
    return x16, x8


def split_mx(x: torch.Tensor):
    """fp32 channels-last image -> MX planes (x16 fp16 image, x8 uint8 [N, H, W, 2 C]) for conv2d(x16, ..., x_mx=x8); C % 64 == 0."""
    _need_cuda(x)
    x = to_channels_last(x)
    n, c, hh, ww = x.shape
    if x.dtype != torch.float32 or c % 64:
        raise L.CrgError("split_mx: fp32 image with C % 64 == 0 expected")
    x16, x8 = _empty_mx(n, c, hh, ww, x.device)
    _call("crg_split_mx", x, _p(x), _p(x16), _p(x8), n * hh * ww, c, MX_X_LOG2[0], MX_X_LOG2[1])
    return x16, x8
