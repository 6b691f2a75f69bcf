"""ControlNet's HED annotator (annot.hip): what follows every conv of the VGG trunk in one pass, and the detector's tail in one launch."""
import ctypes as C
import functools
from typing import Sequence, Tuple

import torch

from .. import _lib as L
from ._base import HALF, _call, _need_cuda, _p, _written, empty_image, f32_vec

HED_MAX_MAPS = 8  # crg_hed_fuse: side maps per call


def _dense_planes(planes, n, c, hh, ww, device, what):
    """None / False -> (None, None); True -> fresh dense channels-last planes; (hi, lo) -> the caller's, which must be dense"""
    if planes is None or planes is False:
        return None, None
    if planes is True:
        return empty_image(n, c, hh, ww, HALF, device), empty_image(n, c, hh, ww, HALF, device)
    hi, lo = planes
    _need_cuda(hi, lo)
    for t in (hi, lo):
        if t.dtype != HALF or tuple(t.shape) != (n, c, hh, ww) or not t.permute(0, 2, 3, 1).is_contiguous():
            raise L.CrgError(f"{what}: a dense channels-last {HALF} plane [{n}, {c}, {hh}, {ww}] expected, got {tuple(t.shape)} {t.dtype} strides {t.stride()}")
    return hi, lo


def relu_pool_proj(x: torch.Tensor, *, planes=None, pool=None, proj=None):
    """Everything that follows one conv of HED's VGG trunk, in one pass over the conv's fp32 output x [N, C, H, W] (channels-last, dense;
    crg_relu_pool_proj).  With r = relu(x), any non-empty subset of
      planes  True or (hi, lo): the half-type planes of r - bitwise split_bf16(F.relu(x)) - the operand of the next conv of the block;
      pool    True or (hi, lo): the planes of F.max_pool2d(r, 2, 2) (odd sizes floor) - the operand of the next block's first conv;
      proj    (weight [1, C, 1, 1] or [C], bias [1] or None): the block's 1 x 1 `projection` conv of r, fp32 [N, 1, H, W].  Its summation
              order depends on C alone - not on the batch, the image size or the batch-invariant mode.
    Returns (planes, pooled planes, projection) with None for what was not asked for.  C % 8 == 0, C <= 2048."""
    pw, pb = (None, None) if proj is None else proj
    _need_cuda(x, pw, pb)
    if x.dim() != 4 or x.dtype != torch.float32:
        raise L.CrgError(f"relu_pool_proj: a 4-D fp32 image expected, got {tuple(x.shape)} {x.dtype}")
    n, c, hh, ww = x.shape
    if not x.permute(0, 2, 3, 1).is_contiguous():
        raise L.CrgError(f"relu_pool_proj: a dense channels-last image expected (a conv's output), got strides {x.stride()}")
    if c % 8 or c < 8 or c > 2048 or min(n, hh, ww) < 1:
        raise L.CrgError(f"relu_pool_proj: C = {c} must be a multiple of 8 (8 .. 2048) and the image non-empty, got {tuple(x.shape)}")
    hi, lo = _dense_planes(planes, n, c, hh, ww, x.device, "relu_pool_proj: planes")
    qhi = qlo = None
    if pool is not None and pool is not False:
        if hh < 2 or ww < 2:
            raise L.CrgError(f"relu_pool_proj: a {hh} x {ww} image has no 2 x 2 window")
        qhi, qlo = _dense_planes(pool, n, c, hh // 2, ww // 2, x.device, "relu_pool_proj: pool")
    w = b = y = None
    if proj is not None:
        if pw.dtype != torch.float32 or pw.numel() != c or (pb is not None and (pb.dtype != torch.float32 or pb.numel() != 1)):
            raise L.CrgError(f"relu_pool_proj: proj = (fp32 weight of {c} values, fp32 bias of one), got {tuple(pw.shape)} {pw.dtype}")
        w = f32_vec(pw.reshape(c) if pw.is_contiguous() else pw.contiguous().reshape(c))
        b = None if pb is None else f32_vec(pb.reshape(1))
        y = torch.empty((n, 1, hh, ww), dtype=torch.float32, device=x.device)
    if hi is None and qhi is None and y is None:
        raise L.CrgError("relu_pool_proj: nothing to write")
    _call("crg_relu_pool_proj", x, _p(x), _p(hi), _p(lo), _p(qhi), _p(qlo), _p(w), _p(b), _p(y), n, hh, ww, c)
    for t in (hi, lo, qhi, qlo):
        if t is not None:
            _written(t)
    return (None if hi is None else (hi, lo)), (None if qhi is None else (qhi, qlo)), y


@functools.lru_cache(maxsize=32)
def _hed_tables_dev(sizes: Tuple[Tuple[int, int], ...], size: Tuple[int, int], device):
    """postprocess.hed_tables of every map, (int32, fp32) [maps * (W + H)] on the device: uploaded once per (sizes, size, device)"""
    from ..postprocess import hed_tables
    H, W = size
    idx, frac = [], []
    for (h, w) in sizes:
        xi, xf = hed_tables(w, W)
        yi, yf = hed_tables(h, H)
        idx += [torch.from_numpy(xi), torch.from_numpy(yi)]
        frac += [torch.from_numpy(xf), torch.from_numpy(yf)]
    return torch.cat(idx).to(torch.int32).to(device), torch.cat(frac).to(torch.float32).to(device)


def hed_fuse(maps: Sequence[torch.Tensor], size: Tuple[int, int], *, return_logit: bool = False):
    """postprocess.hed_fuse_host on the device, equal to its values, one launch (crg_hed_fuse): the side maps - fp32 [N, h_i, w_i] or
    [N, 1, h_i, w_i], 1 .. 8 of them, any sizes - resized bilinearly to size = (H, W), averaged, squashed by the sigmoid in double and
    quantised.  Returns the uint8 edge map [N, H, W], or (edge map, fp32 mean field [N, H, W]) with `return_logit`.  A map that is not
    dense (a strided view) is read through a contiguous copy.  The interpolation tables are built on the host and uploaded once per
    combination of sizes - before a graph capture, as every table of this package."""
    maps = list(maps)
    if not 1 <= len(maps) <= HED_MAX_MAPS:
        raise L.CrgError(f"hed_fuse: {len(maps)} side maps (1 .. {HED_MAX_MAPS})")
    _need_cuda(*maps)
    H, W = int(size[0]), int(size[1])
    if H < 1 or W < 1:
        raise L.CrgError(f"hed_fuse: empty target size {(H, W)}")
    ms = []
    n = None
    for i, m in enumerate(maps):
        if m.dim() == 4 and m.shape[1] == 1:
            m = m[:, 0]
        if m.dim() != 3 or m.dtype != torch.float32 or min(m.shape) < 1:
            raise L.CrgError(f"hed_fuse: side map {i} must be a non-empty fp32 [N, h, w] or [N, 1, h, w], got {tuple(maps[i].shape)} {m.dtype}")
        if n is None:
            n = m.shape[0]
        if m.shape[0] != n or m.device != maps[0].device:
            raise L.CrgError("hed_fuse: the side maps must share the batch and the device")
        ms.append(m.contiguous())
    dev = ms[0].device
    sizes = tuple((int(m.shape[1]), int(m.shape[2])) for m in ms)
    idx, frac = _hed_tables_dev(sizes, (H, W), dev)
    out = torch.empty((n, H, W), dtype=torch.uint8, device=dev)
    mean = torch.empty((n, H, W), dtype=torch.float32, device=dev) if return_logit else None
    k = len(ms)
    ptrs = (C.c_void_p * k)(*[m.data_ptr() for m in ms])
    hs = (C.c_int * k)(*[s[0] for s in sizes])
    ws = (C.c_int * k)(*[s[1] for s in sizes])
    _call("crg_hed_fuse", ms[0], k, ptrs, hs, ws, _p(idx), _p(frac), _p(out), _p(mean), n, H, W)
    return (out, mean) if return_logit else out
