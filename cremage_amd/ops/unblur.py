"""The face unblur / colorize network's own kernels (unblur.hip): the 4 x 4 / stride 2 transposed conv and the post-norm block tail."""
from typing import Optional

import torch

from .. import _lib as L
from ._base import HALF, _call, _need_cuda, _p, _written, empty_image, f32_vec, to_channels_last
from .film import _film_dst, _film_planes, _film_rows
from .side_channels import _gn_rows_of, _gn_stats_of

_GN_ADD_SLICES = 64  # crg_groupnorm_add_act: row slices per (sample, group) at most


def conv_transpose2d(x_hi: torch.Tensor, x_lo: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor] = None, silu: bool = False) -> torch.Tensor:
    """nn.ConvTranspose2d(Cin, Cout, kernel_size=4, stride=2, padding=1) in the fp32 class, one launch of crg_conv_transpose2d for all four
    output parities.  x_hi, x_lo: the two half-type planes [N, Cin, H, W] (channels-last, dense) of an fp32 activation (split_bf16 /
    group_norm_add_act); weight: the module's [Cin, Cout, 4, 4] parameter, its parity image packed once (PACK_CONVT_UP2); bias fp32
    [Cout] or None; `silu`: ConvTransposeAct's activation in the epilogue.  Returns fp32 [N, Cout, 2 H, 2 W] channels-last.
    Cin % 8 == 0, Cout % 4 == 0, any H, W >= 1.  `last_route()` reports kernel 'convt' with the tile (wnt = width / 32, config = height / 32)."""
    _need_cuda(x_hi, x_lo, weight, bias)
    if x_hi.dim() != 4 or x_hi.dtype != HALF or x_lo.dtype != HALF or x_hi.shape != x_lo.shape:
        raise L.CrgError(f"conv_transpose2d: x_hi / x_lo must be two half-type planes of one [N, C, H, W] shape, got {tuple(x_hi.shape)} {x_hi.dtype} and "
                         f"{tuple(x_lo.shape)} {x_lo.dtype}")
    if weight.dtype != torch.float32:
        raise L.CrgError(f"conv_transpose2d: {weight.dtype} weight - fp32 class only")
    x_hi, x_lo = to_channels_last(x_hi), to_channels_last(x_lo)
    n, cin, hh, ww = x_hi.shape
    if weight.dim() != 4 or weight.shape[0] != cin or tuple(weight.shape[2:]) != (4, 4):
        raise L.CrgError(f"conv_transpose2d: a [{cin}, Cout, 4, 4] weight expected (kernel 4, stride 2, padding 1), got {tuple(weight.shape)}")
    cout = weight.shape[1]
    if cin % 8 or cout % 4:
        raise L.CrgError(f"conv_transpose2d: Cin = {cin} must be a multiple of 8 and Cout = {cout} of 4")
    if bias is not None and bias.numel() != cout:
        raise L.CrgError(f"conv_transpose2d: {bias.numel()} bias values for {cout} channels")
    hi, lo = _packed_convt(weight)
    y = empty_image(n, cout, 2 * hh, 2 * ww, torch.float32, x_hi.device)
    _call("crg_conv_transpose2d", x_hi, _p(x_hi), _p(x_lo), _p(hi), _p(lo), _p(f32_vec(bias)), _p(y), n, hh, ww, cin, cout, int(bool(silu)))
    return y


def _packed_convt(weight: torch.Tensor):
    """(hi, lo) planes [4 Cout, 4 Cin] of the parity image, through the weight cache like every packed weight"""
    from ._base import _pack_cache
    from .packing import _pack_source
    r = _pack_cache.get((weight,), (L.PACK_CONVT_UP2, True))
    if r is not None:
        return r
    src = _pack_source(weight)
    cin, cout = src.shape[0], src.shape[1]
    hi = torch.empty((4 * cout, 4 * cin), dtype=HALF, device=weight.device)
    lo = torch.empty_like(hi)
    _call("crg_pack_weight", weight, _p(src), L.F32, L.PACK_CONVT_UP2, cout, cin, 4, _p(hi), _p(lo))
    return _pack_cache.put((weight,), (L.PACK_CONVT_UP2, True), (hi, lo))


def group_norm_add_act(x: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor, groups: int, eps: float, skip: Optional[torch.Tensor] = None,
                       silu: bool = True, out: Optional[torch.Tensor] = None, planes=None, fp32: bool = True):
    """silu?(GroupNorm(x) + skip) of an fp32 channels-last image x in one pass over x and skip (crg_groupnorm_add_act): as the fp32 image
    (`out`: a channels-last tensor, a column slice of a wider one, or - None - a fresh tensor; `fp32=False`: not written) and / or as the
    (hi, lo) half-type planes the next fp32-class conv reads (`planes`: True, or two destinations that share one row stride), which are
    bitwise split_bf16 of the fp32 result.  skip: fp32, same shape, dense or a column slice.  Where x still carries its producing
    conv's statistics side channel the statistics pass over x is replaced by a fold of those partials.  Any C % 8 == 0, up to 64 groups
    of any size, any H * W.  Returns (y, planes), None for what was not asked for."""
    _need_cuda(x, weight, bias, skip, out)
    if x.dim() != 4 or x.dtype != torch.float32:
        raise L.CrgError(f"group_norm_add_act: a 4-D fp32 image expected, got {tuple(x.shape)} {x.dtype}")
    x = to_channels_last(x)
    n, c, hh, ww = x.shape
    if c % 8 or groups < 1 or groups > 64 or c % groups:
        raise L.CrgError(f"group_norm_add_act: {c} channels (a multiple of 8) in {groups} groups (1 .. 64, dividing C)")
    if weight.numel() != c or bias.numel() != c:
        raise L.CrgError(f"group_norm_add_act: {weight.numel()} gains / {bias.numel()} offsets for {c} channels")
    lds = 0
    if skip is not None:
        lds = _film_rows(skip, "group_norm_add_act: skip")[4]
        if tuple(skip.shape) != (n, c, hh, ww):
            raise L.CrgError(f"group_norm_add_act: skip {tuple(skip.shape)} does not match x {tuple(x.shape)}")
    y, ldy = (None, 0)
    if fp32:
        y, ldy = _film_dst(out, n, c, hh, ww, x.device, "group_norm_add_act: out")
    elif out is not None:
        raise L.CrgError("group_norm_add_act: fp32=False takes no `out`")
    hi, lo, ldp = _film_planes(planes, n, c, hh, ww, x.device, "group_norm_add_act")
    if y is None and hi is None:
        raise L.CrgError("group_norm_add_act: nothing to write")
    for t, ld, al, what in ((skip, lds, 4, "skip"), (y, ldy, 4, "out"), (hi, ldp, 8, "planes"), (lo, ldp, 8, "planes")):
        if t is not None and (ld % al or t.data_ptr() % 16):
            raise L.CrgError(f"group_norm_add_act: {what} needs 16-byte aligned rows (row stride {ld}, offset {t.data_ptr() % 16})")
    st = _gn_stats_of(x, hh * ww) if _gn_rows_of(x) == 32 and (hh * ww) % 32 == 0 else None
    ws = torch.empty((n * groups * _GN_ADD_SLICES * 2,), dtype=torch.float64, device=x.device)
    gamma, beta = f32_vec(weight), f32_vec(bias)
    _call("crg_groupnorm_add_act", x, _p(x), _p(skip), lds, _p(gamma), _p(beta), _p(st), _p(y), ldy, _p(hi), _p(lo), ldp, _p(ws), ws.numel() * 8,
          n, hh * ww, c, int(groups), float(eps), int(bool(silu)))
    for t in (y, hi, lo):
        if t is not None:
            _written(t)
    return y, (None if hi is None else (hi, lo))
