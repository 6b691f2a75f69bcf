"""MX8 feed-forward (opt-in).

Block-scaled e4m3 operands for the two feed-forward GEMMs (include/crg_hip.h, "MX8"): q = uint8 e4m3fn codes [R][K], e = uint8 E8M0
scales [R][K / 32], one per 32 elements along K.  Off unless FeedForward(precision="mx8") / cremage_amd.set_ff_precision asks for it;
knobs.FF_MX8 makes "mx8" the default of newly built FeedForward modules.  The *_host functions restate the format in plain torch on the
CPU: they are the reference of the kernels, never a fallback.
"""
import ctypes as C
from typing import Optional, Tuple

import torch

from .. import _lib as L
from ._base import HALF, _call, _dt, _need_cuda, _p, _pack_cache, f32_vec
from .packing import _pack_source, packed_geglu_bias


def quant_mx8_host(x: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """(q uint8 [..., K], e uint8 [..., K / 32]) of x by the MX8 rule, applied to the fp32 value of each element (CPU, plain torch)."""
    x = x.detach().to("cpu", torch.float32)
    K = x.shape[-1]
    if K % 32:
        raise ValueError(f"quant_mx8_host: the last dim must be a multiple of 32, got {K}")
    b = x.reshape(-1, K // 32, 32)
    a = b.abs().amax(-1)
    mant, ex = torch.frexp(a)  # a = mant 2^ex with mant in [0.5, 1): m = 2 mant, E = ex - 1
    e = ex.to(torch.int64) - 1 - 8 + 127 + (mant > 0.875).to(torch.int64)
    e = torch.where(a == 0, torch.full_like(e, 127), e).clamp(0, 254)
    inv = ((254 - e) << 23).to(torch.int32).view(torch.float32)  # 2^(127 - e), exact: e <= 247 for every fp32 a
    v = (b * inv.unsqueeze(-1)).clamp(-448.0, 448.0)
    q = v.to(torch.float8_e4m3fn).view(torch.uint8)
    q = torch.where((q & 0x7F) == 0, torch.zeros_like(q), q)  # a value that rounds to zero keeps no sign
    return q.reshape(x.shape).contiguous(), e.to(torch.uint8).reshape(x.shape[:-1] + (K // 32,)).contiguous()


def dequant_mx8_host(q: torch.Tensor, e: torch.Tensor) -> torch.Tensor:
    """float64 values code * 2^(e - 127) of an MX8 matrix (exact)."""
    q, e = q.detach().cpu(), e.detach().cpu()
    K = q.shape[-1]
    v = q.contiguous().view(torch.float8_e4m3fn).to(torch.float32).to(torch.float64).reshape(-1, K // 32, 32)
    s = torch.ldexp(torch.ones((), dtype=torch.float64), e.reshape(-1, K // 32).to(torch.int64) - 127)
    return (v * s.unsqueeze(-1)).reshape(q.shape)


def linear_mx8_host(x: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor] = None, act: Optional[str] = None,
                    residual: Optional[torch.Tensor] = None) -> torch.Tensor:
    """float64 act(dq(x) dq(w)^T + bias) + residual with both operands quantised along K by the MX8 rule: what linear_mx8 computes up to
    accumulation order and output rounding.  act: None | "geglu" (value = first half of the rows of w, gate = second, erf form)."""
    xd = dequant_mx8_host(*quant_mx8_host(x))
    wd = dequant_mx8_host(*quant_mx8_host(w.detach().reshape(w.shape[0], -1)))
    y = xd @ wd.t()
    if bias is not None:
        y = y + bias.detach().cpu().double()
    if act == "geglu":
        v, g = y.chunk(2, dim=-1)
        y = v * torch.nn.functional.gelu(g)
    elif act is not None:
        raise ValueError(f"linear_mx8_host: act {act!r}")
    if residual is not None:
        y = y + residual.detach().cpu().double()
    return y


def _rows_of(x: torch.Tensor) -> Tuple[torch.Tensor, int]:
    """x as rows of its last dim behind ONE row stride (elements); a view that is not such rows is copied."""
    K = x.shape[-1]
    ok = x.stride(-1) == 1 or K == 1
    for i in range(x.dim() - 2):
        ok = ok and (x.shape[i] == 1 or x.stride(i) == x.stride(i + 1) * x.shape[i + 1])
    if not ok:
        x = x.contiguous()
    return x, (x.stride(-2) if x.dim() >= 2 and x.shape[-2] > 1 else K)


def quant_mx8(x: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """(q, e) of a half-type tensor along its last dim (crg_quant_mx8; bit-exact to quant_mx8_host).  Row-strided views are read in place."""
    _need_cuda(x)
    K = x.shape[-1]
    if x.dtype != HALF or K % 32 or x.numel() == 0:
        raise L.CrgError(f"quant_mx8: a non-empty {HALF} tensor whose last dim is a multiple of 32 expected, got {x.dtype} {tuple(x.shape)}")
    x, ld = _rows_of(x)
    q = torch.empty(x.shape, dtype=torch.uint8, device=x.device)
    e = torch.empty(x.shape[:-1] + (K // 32,), dtype=torch.uint8, device=x.device)
    _call("crg_quant_mx8", x, _p(x), ld, _p(q), _p(e), x.numel() // K, K)
    return q, e


def packed_weight_mx8(w: torch.Tensor, geglu: bool = False) -> Tuple[torch.Tensor, torch.Tensor]:
    """(codes [N, K], scales [N, K / 32]) of a Linear weight as crg_gemm_mx8 reads them (crg_pack_weight_mx8), cached like packed_weight."""
    _need_cuda(w)
    r = _pack_cache.get((w,), ("mx8", geglu))
    if r is not None:
        return r
    src = _pack_source(w.detach().reshape(w.shape[0], -1))
    n_out, n_in = src.shape
    if n_in % 32 or (geglu and n_out % 32):
        raise L.CrgError(f"packed_weight_mx8: weight {tuple(w.shape)} needs K % 32 == 0 (and N % 32 == 0 for GEGLU)")
    wq = torch.empty((n_out, n_in), dtype=torch.uint8, device=w.device)
    we = torch.empty((n_out, n_in // 32), dtype=torch.uint8, device=w.device)
    _call("crg_pack_weight_mx8", w, _p(src), _dt(src), L.PACK_GEGLU if geglu else L.PACK_LINEAR, n_out, n_in, _p(wq), _p(we))
    return _pack_cache.put((w,), ("mx8", geglu), (wq, we))


_MX8_OUT = {"half": L.MX8_OUT_HALF, "f32": L.MX8_OUT_F32, "mx8": L.MX8_OUT_MX8}


def linear_mx8(q: torch.Tensor, e: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor] = None, act: Optional[str] = None,
               residual: Optional[torch.Tensor] = None, out: str = "half"):
    """act(dq(q, e) @ dq(weight)^T + bias) + residual on the block-scaled matrix instruction (crg_gemm_mx8).  (q, e): quant_mx8 or an
    out="mx8" result; weight: [N, K] Linear weight (packed and cached here); act: None | "geglu"; residual: half type, plain epilogue
    only.  out: "half" | "f32" -> one tensor, "mx8" -> (y_q, y_e), the next linear_mx8's operand (output width % 64 == 0).
    K % 64 == 0 and N % 32 == 0; anything else raises - there is no other route."""
    _need_cuda(q, e, weight, bias, residual)
    if out not in _MX8_OUT or act not in (None, "geglu"):
        raise L.CrgError(f"linear_mx8: out {out!r} / act {act!r} unsupported")
    K = q.shape[-1]
    N = weight.shape[0]
    if q.dtype != torch.uint8 or e.dtype != torch.uint8 or e.shape != q.shape[:-1] + (K // 32,) or q.numel() == 0:
        raise L.CrgError(f"linear_mx8: (q, e) must be uint8 planes [..., K] and [..., K / 32], got {tuple(q.shape)} and {tuple(e.shape)}")
    if weight[0].numel() != K:
        raise L.CrgError(f"linear_mx8: weight {tuple(weight.shape)} does not match input width {K}")
    if K % 64 or N % 32:
        raise L.CrgError(f"linear_mx8: K % 64 == 0 and N % 32 == 0 expected, got K {K}, N {N}")
    geglu = act == "geglu"
    n_out = N // 2 if geglu else N
    if out == "mx8" and n_out % 64:
        raise L.CrgError(f"linear_mx8: an MX8 output needs a width that is a multiple of 64, got {n_out}")
    if geglu and residual is not None:
        raise L.CrgError("linear_mx8: the GEGLU epilogue takes no residual")
    q, e = q.contiguous(), e.contiguous()
    M = q.numel() // K
    lead = q.shape[:-1]
    if residual is not None:
        if residual.shape != lead + (n_out,) or residual.dtype != HALF:
            raise L.CrgError(f"linear_mx8: residual must be {HALF} of the output's shape")
        residual = residual.contiguous()
    wq, we = packed_weight_mx8(weight, geglu)
    b = None if bias is None else (packed_geglu_bias(bias) if geglu else f32_vec(bias))
    y_e = None
    if out == "mx8":
        y = torch.empty(lead + (n_out,), dtype=torch.uint8, device=q.device)
        y_e = torch.empty(lead + (n_out // 32,), dtype=torch.uint8, device=q.device)
    else:
        y = torch.empty(lead + (n_out,), dtype=HALF if out == "half" else torch.float32, device=q.device)
    a = L.Mx8GemmArgs(a_q=q.data_ptr(), lda=K, a_e=e.data_ptr(), lde=K // 32, w_q=wq.data_ptr(), w_e=we.data_ptr(), bias=_p(b).value,
                      residual=_p(residual).value, ldr=n_out, y=y.data_ptr(), ldy=n_out, y_e=_p(y_e).value, ldye=n_out // 32,
                      M=M, N=N, K=K, epilogue=L.EPI_GEGLU if geglu else L.EPI_NONE, y_kind=_MX8_OUT[out])
    _call("crg_gemm_mx8", q, C.byref(a))
    return (y, y_e) if out == "mx8" else y


def ff_mx8_ok(x: torch.Tensor, w1: torch.Tensor, w2: torch.Tensor) -> bool:
    """Shapes the MX8 feed-forward chain takes: half-type x [..., K] on the device, w1 [2 F, K] (GEGLU projection), w2 [N, F] with
    K % 64 == 0, F % 64 == 0 (the intermediate is an MX8 output) and N % 32 == 0."""
    if not (x.is_cuda and x.dtype == HALF and x.numel() > 0 and w1.is_cuda and w2.is_cuda):
        return False
    K = x.shape[-1]
    n1, n2 = w1.shape[0], w2.shape[0]
    return K % 64 == 0 and n1 % 128 == 0 and w1[0].numel() == K and w2[0].numel() == n1 // 2 and n2 % 32 == 0
