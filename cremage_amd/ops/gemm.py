"""The GEMM family: linear, the LayerNorm + GEMM routes and the transposed projections."""
import ctypes as C
import math
from typing import Optional

import torch

from .. import _lib as L, knobs
from ._base import _DT, HALF, _act_dt, _call, _h, _need_cuda, _p, _prec, _st, f32_vec
from .norms import layer_norm
from .packing import packed_geglu_bias, packed_ln_weight, packed_weight
from .side_channels import _gn_stats_buffer, _ln_stats_of, ln_epi_ok, row_stats_parts


def _gemm(h, **kw):
    a = L.GemmArgs()
    for k, v in kw.items():
        setattr(a, k, v)
    L.check(L.load().crg_gemm(h, _st(), C.byref(a)), h, "crg_gemm")


def rows_per_sample(x: torch.Tensor, gn_hw: Optional[int] = None) -> int:
    """crg_gemm_args.rows_per_sample of a GEMM over the last dim of x (read under the batch-invariant mode only): the rows of one
    sample - gn_hw where the caller names the image size, T for [B, T, K] tokens (every dim between the first and the last), 1 for
    2-D inputs such as the hoisted time rows, whose rows are samples."""
    if gn_hw:
        return int(gn_hw)
    return 1 if x.dim() <= 2 else int(math.prod(x.shape[1:-1]))


def last_route(device: Optional[int] = None) -> dict:
    """What the last crg_gemm / crg_conv2d call on the device's context decided (crg_last_route, include/crg_hip.h): a plain dict with
    `kernel` in L.ROUTE_KERNELS, `reduce` in L.ROUTE_REDUCES and the other fields of crg_route as integers.  Host bookkeeping: reads
    nothing from the device.  linear / linear_transposed / conv1x1 / conv2d set it; the thin-channel convs (crg_conv_small), ln_linear
    and linear_mx8 have one kernel each and leave it as it was."""
    h = L.ctx(torch.cuda.current_device() if device is None else int(device))
    r = L.Route()
    L.check(L.load().crg_last_route(h, C.byref(r)), h, "crg_last_route")
    d = {name: int(getattr(r, name)) for name, _ in L.Route._fields_}
    d["kernel"] = L.ROUTE_KERNELS[d["kernel"]]
    d["reduce"] = L.ROUTE_REDUCES[d["reduce"]]
    return d


def linear(x: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor] = None, residual: Optional[torch.Tensor] = None,
           act: Optional[str] = None, out_dtype: Optional[torch.dtype] = None, gn_hw: Optional[int] = None,
           transposed_from: Optional[int] = None, row_stats: bool = False, ln=None):
    """y = act(x @ weight^T + bias) + residual over the last dim of x.
    weight: [N, K] (nn.Linear) or [N, K, 1, 1] (1x1 conv).  act: None | 'silu' | 'geglu'.
    gn_hw: y (as an image of gn_hw tokens per sample) feeds a GroupNorm - emit its statistics side channel (bf16 only, side_channels.py).
    transposed_from = n0 (test linear_transposed_ok first; x must be [B, T, K]): output columns >= n0 are returned as a SECOND tensor
    [B, N - n0, ld], ld = roundup(T, 8), transposed per sample - the V^T operand of `attention` out of the same launch as Q | K; the
    first tensor then has n0 columns.
    row_stats: y feeds an nn.LayerNorm - emit its row-statistics side channel where the path supports it (bf16, plain epilogue).
    ln = (gamma, beta, eps) (test ln_epi_ok first): y = act(LayerNorm(x) @ weight^T + bias) with the LayerNorm carried as an epilogue
    correction on the statistics x brought along; x itself is read raw, the normalised tensor never exists."""
    _need_cuda(x, weight, bias, residual)
    ln_stats = None
    if ln is not None:
        if not ln_epi_ok(x, weight, act) or residual is not None or gn_hw is not None or out_dtype not in (None, HALF):
            raise L.CrgError("linear: ln= outside its domain (test ln_epi_ok; no residual / GroupNorm statistics / fp32 output)")
        ln_stats = _ln_stats_of(x)
    x = x.contiguous()
    K = x.shape[-1]
    M = x.numel() // K
    N = weight.shape[0]
    if weight[0].numel() != K:
        raise L.CrgError(f"linear: weight {tuple(weight.shape)} does not match input width {K}")
    split = x.dtype == torch.float32
    out_dtype = out_dtype or x.dtype
    if split and out_dtype != torch.float32:
        raise L.CrgError("linear: fp32 (BF16X3) inputs produce fp32 outputs")
    geglu = act == "geglu"
    if ln is not None:  # b: W beta + bias, already in the packed row order
        (hi, ln_s, b), lo = packed_ln_weight(weight, ln[0], ln[1], bias, geglu), None
    else:
        (hi, lo), ln_s = packed_weight(weight, L.PACK_GEGLU if geglu else L.PACK_LINEAR, split), None
        b = None if bias is None else (packed_geglu_bias(bias) if geglu else f32_vec(bias))
    n_out = N // 2 if geglu else N
    vt, vt_tokens, vt_ld = None, 0, 0
    if transposed_from is not None:
        if not linear_transposed_ok(x, weight, transposed_from) or act is not None or residual is not None or gn_hw is not None:
            raise L.CrgError("linear: transposed_from outside its domain (test linear_transposed_ok; no activation / residual / statistics)")
        n_out, vt_tokens = transposed_from, x.shape[1]
        vt_ld = (vt_tokens + 7) // 8 * 8
        vt = torch.empty((x.shape[0], N - transposed_from, vt_ld), dtype=x.dtype, device=x.device)
        if vt_ld != vt_tokens:
            vt[:, :, vt_tokens:].zero_()
    y = torch.empty(x.shape[:-1] + (n_out,), dtype=out_dtype, device=x.device)
    if residual is not None:
        residual = residual.contiguous()
        if residual.shape != y.shape or residual.dtype != y.dtype:
            raise L.CrgError("linear: residual must match the output in shape and dtype")
    h = _h(x)
    rps = rows_per_sample(x, gn_hw)
    stats = _gn_stats_buffer(M, N, gn_hw, x.dtype, out_dtype, x.device) if not geglu else None
    rs = None
    if row_stats and knobs.LN_EPI and stats is None and ln is None and act is None and vt is None and x.dtype == HALF and out_dtype == HALF \
            and N % 8 == 0 and row_stats_parts(N) <= 16:
        rs = torch.empty((M, row_stats_parts(N), 2), dtype=torch.float32, device=x.device)
    _gemm(h, a=x.data_ptr(), lda=K, a_bstride=0, w=hi.data_ptr(), ldw=K, w_bstride=0, w_lo=_p(lo).value, bias=_p(b).value,
          bias_mode=L.BIAS_COL if b is not None else L.BIAS_NONE, residual=_p(residual).value, ldr=n_out, r_bstride=0, y=y.data_ptr(), ldy=n_out, y_bstride=0,
          M=M, N=N, K=K, batch=1, epilogue={None: L.EPI_NONE, "silu": L.EPI_SILU, "geglu": L.EPI_GEGLU}[act], a_dtype=_act_dt(x), y_dtype=_DT[out_dtype],
          prec=_prec(x), a_is_weight=0, a_lo=None, gn_stats=_p(stats).value, vt=_p(vt).value, vt_n0=transposed_from or 0, vt_tokens=vt_tokens, vt_ld=vt_ld,
          row_stats=_p(rs).value, row_stats_parts=rs.shape[1] if rs is not None else 0, ln_stats=_p(ln_stats).value,
          ln_parts=ln_stats.shape[1] if ln_stats is not None else 0, ln_colsum=_p(ln_s).value, ln_eps=float(ln[2]) if ln is not None else 0.0, rows_per_sample=rps)
    if stats is not None:
        y._crg_gn_pending = stats  # the caller that shapes y into an image attaches it (image_of_stats)
    if rs is not None:
        y._crg_ln = (rs, y._version)
    return (y, vt) if vt is not None else y


def ln_linear_auto(x: torch.Tensor, ln, weight: torch.Tensor, bias: Optional[torch.Tensor] = None, act: Optional[str] = None, transposed_from: Optional[int] = None):
    """act(LayerNorm(x) @ weight^T + bias) by the cheapest route the shapes allow (`ln`: an nn.LayerNorm-like module with weight / bias /
    eps, or None for no norm): the epilogue correction when x carries its producer's row statistics, the row-resident kernel for
    K = 320, else layer_norm + linear.  `transposed_from`: the caller has tested linear_transposed_ok (or ln_linear_ok) for it."""
    if ln is None:
        return linear(x, weight, bias, act=act, transposed_from=transposed_from)
    if ln_epi_ok(x, weight, act) and (transposed_from is None or linear_transposed_ok(x, weight, transposed_from)):
        return linear(x, weight, bias, act=act, transposed_from=transposed_from, ln=(ln.weight, ln.bias, ln.eps))
    if ln_linear_ok(x, weight, act, transposed_from):
        return ln_linear(x, ln.weight, ln.bias, ln.eps, weight, bias, act=act, transposed_from=transposed_from)
    return linear(layer_norm(x, ln.weight, ln.bias, ln.eps), weight, bias, act=act, transposed_from=transposed_from)


def linear_transposed_ok(x: torch.Tensor, weight: torch.Tensor, n0: int) -> bool:
    """Shapes `linear(..., transposed_from=n0)` takes: [B, T, K] tokens in the library's half type, N and n0 on tile boundaries of the
    paired epilogue (tile = 160 columns when N % 160 == 0, else 128), K below crg_gemm's split-K rule (the transposed range comes out of
    the GEMM's own epilogue, not out of a reduce pass)."""
    if not (x.is_cuda and x.dim() == 3 and x.dtype == HALF):
        return False
    N, K = weight.shape[0], weight[0].numel()
    bn = 160 if N % 160 == 0 else 128
    return K == x.shape[-1] and K % 8 == 0 and K < 24 * 64 and N % 8 == 0 and 0 < n0 < N and n0 % bn == 0 and N > 32


def ln_linear_ok(x: torch.Tensor, weight: torch.Tensor, act: Optional[str] = None, transposed_from: Optional[int] = None) -> bool:
    """Every precondition crg_ln_gemm enforces (the row-resident LayerNorm + GEMM kernel), so that callers can route on this
    predicate ALONE and fall back to layer_norm + linear otherwise: bf16 tokens of width 320; N a multiple of 8 (GEGLU: of 32,
    packed value / gate groups); a transposed column range starts on a tile boundary (tile = 160 columns when N % 160 == 0, else
    128) of a [B, T, K] input without activation; x, w and y (and the V^T output) each below 2 GiB."""
    if not (x.is_cuda and x.dtype == HALF and x.shape[-1] == 320 and weight[0].numel() == 320):
        return False
    N = weight.shape[0]
    M = x.numel() // 320
    geglu = act == "geglu"
    if act not in (None, "geglu") or N % (32 if geglu else 8):
        return False
    n_out = N // 2 if geglu else N
    if transposed_from is not None:
        bn = 160 if N % 160 == 0 else 128
        if geglu or x.dim() != 3 or not (0 < transposed_from < N) or transposed_from % bn:
            return False
        ld = (x.shape[1] + 7) // 8 * 8
        if x.shape[0] * (N - transposed_from) * ld * 2 >= (1 << 31) and not L.invariant():
            return False
        n_out = transposed_from
    # (batch-invariant mode: the 2 GiB clauses read the size of the whole call, so there they are crg_ln_gemm's errors, not another route)
    return L.invariant() > 0 or max(M * 320, N * 320, M * n_out) * 2 < (1 << 31)


def ln_linear(x: torch.Tensor, ln_weight, ln_bias, eps: float, weight: torch.Tensor, bias: Optional[torch.Tensor] = None,
              act: Optional[str] = None, transposed_from: Optional[int] = None, residual: Optional[torch.Tensor] = None):
    """y = act(LayerNorm(x) @ weight^T + bias) in ONE launch (crg_ln_gemm): nn.LayerNorm + the Linear behind it.
    act: None | 'geglu'.  Falls back to nothing - callers test ln_linear_ok() and otherwise run layer_norm + linear.
    transposed_from = n0 (x must be [B, T, K]): output columns >= n0 are returned as a second tensor [B, N - n0, ld] with
    ld = roundup(T, 8), i.e. transposed per sample (the V^T operand of `attention`); the first tensor then has n0 columns.
    ln_weight = ln_bias = None: no LayerNorm (row-resident plain GEMM); `residual` ([.., N], bf16) is added after the bias."""
    _need_cuda(x, ln_weight, ln_bias, weight, bias)
    if not ln_linear_ok(x, weight, act, transposed_from):
        raise L.CrgError("ln_linear: shape outside the row-resident kernel's domain (test ln_linear_ok, else layer_norm + linear)")
    x = x.contiguous()
    K = x.shape[-1]
    M = x.numel() // K
    N = weight.shape[0]
    geglu = act == "geglu"  # (ln_linear_ok has refused every other activation, and a transposed range on anything but plain [B, T, K] tokens)
    hi, _ = packed_weight(weight, L.PACK_GEGLU if geglu else L.PACK_LINEAR, False)
    n_out = N // 2 if geglu else (transposed_from if transposed_from is not None else N)
    y = torch.empty(x.shape[:-1] + (n_out,), dtype=x.dtype, device=x.device)
    b = None if bias is None else (packed_geglu_bias(bias) if geglu else f32_vec(bias))
    vt, tokens, ld = None, 0, 0
    if transposed_from is not None:
        tokens = x.shape[1]
        ld = (tokens + 7) // 8 * 8
        vt = torch.empty((x.shape[0], N - transposed_from, ld), dtype=x.dtype, device=x.device)
        if ld != tokens:
            vt[:, :, tokens:].zero_()
    if residual is not None:
        residual = residual.contiguous()
        if residual.shape != y.shape or residual.dtype != y.dtype:
            raise L.CrgError("ln_linear: residual must match the output in shape and dtype")
    a = L.LnGemmArgs(x=x.data_ptr(), ldx=K, gamma=_p(f32_vec(ln_weight)).value, beta=_p(f32_vec(ln_bias)).value, eps=float(eps),
                     w=hi.data_ptr(), ldw=K, bias=_p(b).value, y=y.data_ptr(), ldy=n_out, M=M, N=N, K=K, epilogue=L.EPI_GEGLU if geglu else L.EPI_NONE,
                     vt=_p(vt).value, vt_n0=transposed_from or 0, vt_tokens=tokens, vt_ld=ld, residual=_p(residual).value, ldr=n_out)
    _call("crg_ln_gemm", x, C.byref(a))
    return (y, vt) if transposed_from is not None else y


def linear_transposed(x: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out[b] = weight @ x[b]^T (+ bias per row): [B, T, K] tokens -> [B, N, ld] with ld = roundup(T, 8).
    Emits the V projection already transposed ([channel][key]) for crg_attention; pad columns are
    never read unmasked (the kernel masks keys >= T)."""
    _need_cuda(x, weight, bias)
    x = x.contiguous()
    B, T, K = x.shape
    N = weight.shape[0]
    split = x.dtype == torch.float32
    hi, lo = packed_weight(weight, L.PACK_LINEAR, split)
    ld = (T + 7) // 8 * 8
    y = torch.empty((B, N, ld), dtype=x.dtype, device=x.device)
    if ld != T:
        y[:, :, T:].zero_()
    b = f32_vec(bias)
    h = _h(x)
    xh, xl = x, None  # A := weight (packed), W := activations: bf16 rows are already the "packed" layout
    if split:  # fp32 activations cannot sit on the pre-split W side: split them once on the fly (crg_split_bf16, no torch arithmetic)
        xh, xl = torch.empty(x.shape, dtype=HALF, device=x.device), torch.empty(x.shape, dtype=HALF, device=x.device)
        _call("crg_split_bf16", x, _p(x), _p(xh), _p(xl), x.numel())
    # (a_is_weight: the samples lie along `batch` and the rows are the weight's, so rows_per_sample is not read: left 0)
    _gemm(h, a=hi.data_ptr(), lda=K, a_bstride=0, a_lo=_p(lo).value, w=xh.data_ptr(), w_lo=_p(xl).value, ldw=K, w_bstride=T * K,
          bias=_p(b).value, bias_mode=L.BIAS_ROW if b is not None else L.BIAS_NONE, residual=None, ldr=0, r_bstride=0,
          y=y.data_ptr(), ldy=ld, y_bstride=N * ld, M=N, N=T, K=K, batch=B, epilogue=L.EPI_NONE, a_dtype=L.BF16,
          y_dtype=L.F32 if split else L.BF16, prec=L.PREC_BF16X3 if split else L.PREC_BF16, a_is_weight=1)
    return y
