"""GroupNorm, LayerNorm and the in-place row softmax."""
from typing import Optional

import torch

from .. import _lib as L
from ._base import HALF, _act_dt, _call, _need_cuda, _p, _written, empty_image, f32_vec, to_channels_last
from .packing import MX_X_LOG2, _empty_mx
from .side_channels import _gn_rows_of, _gn_stats_of


def group_norm(x: torch.Tensor, weight, bias, groups: int, eps: float, silu: bool = False, x2: Optional[torch.Tensor] = None, split: bool = False):
    """GroupNorm(+SiLU) over a channels-last image; `x2` = second half of a virtual channel concat.  With `split` (fp32
    inputs only) the result is returned as the pair of bf16 planes (hi, lo) that conv2d(hi, ..., x_lo=lo) consumes."""
    _need_cuda(x, weight, bias, x2)
    x = to_channels_last(x)
    n, c1, hh, ww = x.shape
    c = c1
    if x2 is not None:
        x2 = to_channels_last(x2)
        if x2.shape[0] != n or x2.shape[2:] != x.shape[2:] or x2.dtype != x.dtype:
            raise L.CrgError("group_norm: concat halves disagree in shape/dtype")
        c = c1 + x2.shape[1]
    if weight.numel() != c:
        raise L.CrgError(f"group_norm: {weight.numel()} gains for {c} channels")
    gamma, beta = _p(f32_vec(weight)), _p(f32_vec(bias))
    if split == "mx":  # MX planes for the fp32-class 3x3 conv (CRG_PREC_F16MX)
        if x.dtype != torch.float32 or x2 is not None or c % 64:
            raise L.CrgError("group_norm(split='mx'): one fp32 input with C % 64 == 0 expected")
        y16, y8 = _empty_mx(n, c, hh, ww, x.device)
        st1 = _gn_stats_of(x, hh * ww)
        _call("crg_groupnorm_mx", x, _p(x), _p(st1), gamma, beta, _p(y16), _p(y8), n, hh * ww, c, groups, eps, int(silu), MX_X_LOG2[0], MX_X_LOG2[1])
        return y16, y8
    if split:
        if x.dtype != torch.float32:
            raise L.CrgError("group_norm(split=True) is the fp32-class path: fp32 input expected")
        hi, lo = empty_image(n, c, hh, ww, HALF, x.device), empty_image(n, c, hh, ww, HALF, x.device)
        st1 = _gn_stats_of(x, hh * ww) if x2 is None else None
        if st1 is not None:  # statistics handed over by the fp32-class conv that produced x: no statistics pass over the fp32 tensor
            _call("crg_groupnorm_pre_split", x, _p(x), _p(st1), gamma, beta, _p(hi), _p(lo), n, hh * ww, c, groups, eps, int(silu))
        else:
            _call("crg_groupnorm_split", x, _p(x), _p(x2), c1, gamma, beta, _p(hi), _p(lo), n, hh * ww, c, groups, eps, int(silu))
        return hi, lo
    y = empty_image(n, c, hh, ww, x.dtype, x.device)
    if x.dtype == HALF:
        # statistics handed over by the producer(s) of x (and x2): no statistics pass over the tensor
        st1 = _gn_stats_of(x, hh * ww)
        st2 = _gn_stats_of(x2, hh * ww) if x2 is not None else None
        if st1 is not None and (x2 is None or st2 is not None):
            _call("crg_groupnorm_pre", x, _p(x), _p(x2), c1, _p(st1), _p(st2), gamma, beta, _p(y), n, hh * ww, c, groups, eps, int(silu), L.BF16,
                  _gn_rows_of(x), _gn_rows_of(x2))
            return y
    _call("crg_groupnorm", x, _p(x), _p(x2), c1, gamma, beta, _p(y), n, hh * ww, c, groups, eps, int(silu), _act_dt(x))
    return y


def layer_norm(x: torch.Tensor, weight, bias, eps: float = 1e-5):
    _need_cuda(x, weight, bias)
    x = x.contiguous()
    dim = x.shape[-1]
    y = torch.empty_like(x)
    _call("crg_layernorm", x, _p(x), _p(f32_vec(weight)), _p(f32_vec(bias)), _p(y), x.numel() // dim, dim, eps, _act_dt(x))
    return y


def softmax_rows_(x: torch.Tensor, cols: int, scale: float):
    """In-place softmax(x[..., :cols] * scale) over the last dim of contiguous rows of stride x.shape[-1].  It writes through the raw
    pointer, so it cannot repair a layout by copying: a view that is not contiguous rows raises."""
    _need_cuda(x)
    if x.dim() < 1 or not x.is_contiguous():
        raise L.CrgError(f"softmax_rows_: contiguous rows expected, got shape {tuple(x.shape)} with strides {x.stride()}")
    ld = x.shape[-1]
    if not 0 < cols <= ld:
        raise L.CrgError(f"softmax_rows_: {cols} columns in rows of {ld}")
    _call("crg_softmax_rows", x, _p(x), _p(x), x.numel() // ld, cols, ld, scale, _act_dt(x))
    return _written(x)
