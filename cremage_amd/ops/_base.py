"""What every family module of `cremage_amd.ops` builds on: dtype codes, the launch helper, the weight caches, the layout helpers, profiling."""
import ctypes as C
from typing import Optional

import torch

from .. import _lib as L

# The library's 16-bit type: bfloat16 (default) or, with CRG_HALF=f16, IEEE fp16 (the fp16-operand build of the same kernels).
# Code L.BF16 in a dtype argument means "the library's half type" in both builds.
HALF = torch.float16 if L.HALF_F16 else torch.bfloat16
_DT = {HALF: L.BF16, torch.float32: L.F32}
if not L.HALF_F16:
    _DT[torch.float16] = L.F16  # weight sources only (crg_pack_weight converts)


def _dt(t: torch.Tensor) -> int:
    try:
        return _DT[t.dtype]
    except KeyError:
        raise L.CrgError(f"unsupported dtype {t.dtype}")


def _act_dt(t: torch.Tensor) -> int:
    if t.dtype not in (HALF, torch.float32):
        raise L.CrgError(f"activations must be {HALF} or float32, got {t.dtype}")
    return _DT[t.dtype]


def _prec(t: torch.Tensor) -> int:
    return L.PREC_BF16 if t.dtype == HALF else L.PREC_BF16X3


def _need_cuda(*ts):
    for t in ts:
        if t is not None and not t.is_cuda:
            raise L.CrgError("cremage_amd.ops: tensors must live on a HIP device (no CPU fallback exists)")


def _h(t: torch.Tensor):
    """crg context of the tensor's device.  Launches go to torch's CURRENT stream (`_st`), which belongs to the current device: a
    tensor on another device would have its pointers handed to the wrong GPU's queue, so that is an error, not a silent launch
    (multi-GPU runs are one process per GPU; a process driving several sets `torch.cuda.device(t.device)` around its calls)."""
    cur = torch.cuda.current_device()
    idx = t.device.index if t.device.index is not None else cur
    if idx != cur:
        raise L.CrgError(f"tensor lives on cuda:{idx} but the current device is cuda:{cur}: wrap the call in torch.cuda.device(...)")
    return L.ctx(idx)


def _st():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _call(name: str, t: torch.Tensor, *args) -> None:
    """One launch of the library's entry point `name`: on the context of t's device (`_h`) and torch's current stream, its status checked
    under the symbol's name.  A struct-argument entry point takes `C.byref(a)` as an ordinary argument."""
    h = _h(t)
    L.check(getattr(L.load(), name)(h, _st(), *args), h, name)


def _p(t: Optional[torch.Tensor]):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def _is_dense(t: torch.Tensor) -> bool:
    """Non-overlapping and dense: the tensor's elements are exactly the numel() consecutive ones behind data_ptr(), in some order of the
    dims (contiguous, channels-last, ...).  What an elementwise kernel that walks numel() elements from the raw pointer needs; a slice
    (gaps) or an expanded dim (stride 0) is not."""
    want = 1
    for size, stride in sorted(((sz, st) for sz, st in zip(t.shape, t.stride()) if sz != 1), key=lambda p: p[1]):
        if stride != want:
            return False
        want *= size
    return True


def _written(t: torch.Tensor) -> torch.Tensor:
    """A kernel of this library just wrote `t` in place through its raw pointer: tell PyTorch (bump `_version`), so that everything keyed
    on the version - the GroupNorm statistics riding on the tensor (`_crg_gn`), the cross-attention K / V cache, the weight caches -
    sees the write as it sees a torch in-place op.  A raw write through a VIEW bumps the shared counter of the base as well."""
    torch.autograd.graph.increment_version(t)
    for a in ("_crg_gn", "_crg_ln"):
        if hasattr(t, a):
            delattr(t, a)
    return t


# ---------------------------------------------------------------------------------- weight cache
class TensorKeyedCache:
    """Cache of values derived from torch tensors (packed weights, fp32 copies, merged LoRA weights).

    An entry is keyed on the IDENTITY of its source tensors (id + weakref) and stamped with their (data_ptr, _version, dtype, device): it
    is hit only while the very same tensor objects still hold the very same, unmodified storage.  Keying on data_ptr alone would be wrong
    - the caching allocator hands the address of a freed parameter to the next model's parameter of the same shape.  Entries die with
    their sources (weakref callbacks), so `load_state_dict` (in-place copy -> _version bump), LoRA `setattr` of fresh Parameters
    (image_generator.py:408-453) and `.to()/.half()` (new storage) all invalidate correctly."""

    def __init__(self, max_entries: int = 8192):
        self._d = {}
        self._max = max_entries

    @staticmethod
    def _stamp(t: torch.Tensor):
        return (t.data_ptr(), t._version, t.dtype, t.device, tuple(t.shape))

    def get(self, tensors, extra=()):
        key = (tuple(id(t) for t in tensors), extra)
        e = self._d.get(key)
        if e is None:
            return None
        refs, stamps, value = e
        for t, r, st in zip(tensors, refs, stamps):
            if r() is not t or self._stamp(t) != st:
                self._d.pop(key, None)
                return None
        return value

    def put(self, tensors, extra, value):
        import weakref
        if len(self._d) >= self._max:
            self.clear()
        key = (tuple(id(t) for t in tensors), extra)

        def _drop(_ref, key=key, d=self._d):
            d.pop(key, None)

        self._d[key] = (tuple(weakref.ref(t, _drop) for t in tensors), tuple(self._stamp(t) for t in tensors), value)
        TensorKeyedCache.epoch += 1
        return value

    # bumped whenever ANY derived weight image is (re)built or a Parameter is registered: cremage_amd.graphs re-lists the module's
    # parameters when it moves (the weight stamp itself is the parameters' (data_ptr, _version))
    epoch = 0
    # bumped whenever ANY cache DROPS its values (clear(), or the overflow clear in put()): a captured hipGraph bakes in the
    # addresses of the packed / stacked / merged images it was warmed up with, and those are freed here while the parameters -
    # and with them the weight stamp - stay what they were.  The generation is part of the stamp, so such a graph is re-captured.
    generation = 0

    def clear(self):
        self._d.clear()
        TensorKeyedCache.generation += 1


_pack_cache = TensorKeyedCache()
_f32_cache = TensorKeyedCache()


def clear_weight_cache():
    _pack_cache.clear()
    _f32_cache.clear()


def f32_vec(v: Optional[torch.Tensor]) -> Optional[torch.Tensor]:
    """fp32 contiguous view/copy of a bias / norm gain (kernels take fp32 vectors)."""
    if v is None:
        return None
    if v.dtype == torch.float32 and v.is_contiguous():
        return v.detach()
    r = _f32_cache.get((v,))
    if r is None:
        r = _f32_cache.put((v,), (), v.detach().float().contiguous())
    return r


# ---------------------------------------------------------------------------------- layout helpers
def to_channels_last(x: torch.Tensor) -> torch.Tensor:
    """No-op for tensors that already have NHWC strides; otherwise one boundary transpose kernel."""
    if x.dim() != 4:
        raise L.CrgError(f"expected a 4-D image tensor, got shape {tuple(x.shape)}")
    if x.permute(0, 2, 3, 1).is_contiguous():
        return x
    return nchw_to_nhwc(x.contiguous(), x.dtype)


def empty_image(n, c, h, w, dtype, device) -> torch.Tensor:
    return torch.empty((n, h, w, c), dtype=dtype, device=device).permute(0, 3, 1, 2)


def tokens_of(x: torch.Tensor) -> torch.Tensor:
    """[N, C, H, W] channels-last image -> [N, H*W, C] contiguous view (no copy)."""
    n, c, h, w = x.shape
    return x.permute(0, 2, 3, 1).reshape(n, h * w, c)


def image_of(t: torch.Tensor, h: int, w: int) -> torch.Tensor:
    """[N, H*W, C] tokens -> [N, C, H, W] channels-last view (no copy)."""
    n, hw, c = t.shape
    return t.reshape(n, h, w, c).permute(0, 3, 1, 2)


def image_of_stats(t: torch.Tensor, h: int, w: int) -> torch.Tensor:
    """image_of() that carries the GroupNorm statistics `linear(..., gn_hw=h*w)` produced over to the image view."""
    img = image_of(t, h, w)
    st = getattr(t, "_crg_gn_pending", None)
    if st is not None:
        img._crg_gn = (st, img._version, h * w)
    return img


def nchw_to_nhwc(x: torch.Tensor, dtype: torch.dtype, x2: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Contiguous NCHW tensor -> channels-last tensor of `dtype` (one transpose+cast kernel).  `x2` [N, C2, H, W]: the result is
    cat([x, x2], dim 1) (crg_nchw2_to_nhwc: the concat is folded into the same launch, no concatenated tensor is built)."""
    _need_cuda(x, x2)
    n, c, hh, ww = x.shape
    if x.dtype not in (torch.float32, HALF):
        x = x.float()
    x = x.contiguous()
    if x2 is None:
        y = empty_image(n, c, hh, ww, dtype, x.device)
        _call("crg_nchw_to_nhwc", x, _p(x), _p(y), n, c, hh * ww, _act_dt(x), _DT[dtype])
        return y
    if x2.dim() != 4 or x2.shape[0] != n or tuple(x2.shape[2:]) != (hh, ww):
        raise L.CrgError(f"nchw_to_nhwc: second source {tuple(x2.shape)} does not match {tuple(x.shape)} in batch and size")
    x2 = x2.to(x.dtype).contiguous()
    y = empty_image(n, c + x2.shape[1], hh, ww, dtype, x.device)
    _call("crg_nchw2_to_nhwc", x, _p(x), _p(x2), _p(y), n, c, x2.shape[1], hh * ww, _act_dt(x), _DT[dtype])
    return y


def nhwc_to_nchw(x: torch.Tensor, dtype: torch.dtype) -> torch.Tensor:
    """Channels-last tensor -> contiguous NCHW tensor of `dtype`."""
    _need_cuda(x)
    x = to_channels_last(x)
    n, c, hh, ww = x.shape
    y = torch.empty((n, c, hh, ww), dtype=dtype, device=x.device)
    _call("crg_nhwc_to_nchw", x, _p(x), _p(y), n, c, hh * ww, _act_dt(x), _DT[dtype])
    return y


# ---------------------------------------------------------------------------------- profiling
class profile:
    """Context manager: per-kernel device time (HIP events on the launch stream) + algorithmic FLOPs/bytes of every kernel launched by
    crg_* calls inside it (bench.py's `roofline`).  `kernels` is keyed by kernel slot (one per kernel symbol, with its rocprofv3 name),
    `result` sums the slots into families."""

    def __init__(self, device=None):
        self.dev = torch.cuda.current_device() if device is None else device
        self.result = None

    def __enter__(self):
        h = L.ctx(self.dev)
        L.check(L.load().crg_profile_begin(h), h, "crg_profile_begin")
        return self

    def __exit__(self, *exc):
        h = L.ctx(self.dev)
        p = L.Profile()
        L.check(L.load().crg_profile_end(h, _st(), C.byref(p)), h, "crg_profile_end")
        self.kernels = {L.SLOT_NAMES[i]: dict(ms=p.ms[i], flops=p.flops[i], bytes=p.bytes[i], launches=p.launches[i],
                                              symbol=L.load().crg_kernel_name(i).decode(), family=L.SLOT_FAMILY[i])
                        for i in range(L.K_SLOTS)}
        self.result = {}
        for k in self.kernels.values():
            f = self.result.setdefault(k["family"], dict(ms=0.0, flops=0.0, bytes=0.0, launches=0))
            for key in ("ms", "flops", "bytes", "launches"):
                f[key] += k[key]
        return False
