"""Attention: half-type flash kernels, fp32-class flash kernel, unfused GEMM + softmax route (`attn`, not `attention`: that name is the exported function's)."""
import ctypes as C
from typing import Optional

import torch

from .. import _lib as L, knobs
from ._base import HALF, _act_dt, _call, _h, _need_cuda, _p
from .gemm import _gemm
from .norms import softmax_rows_


def _attention_x3_why_not(q, k, vt, heads):
    """The violated condition of the fp32 flash kernel's domain, or None."""
    for name, t in (("q", q), ("k", k), ("vt", vt)):
        if not t.is_cuda:
            return f"{name} does not live on a HIP device"
        if t.dtype != torch.float32:
            return f"{name} is {t.dtype}, the kernel takes float32 only"
    if q.dim() != 3 or heads <= 0 or q.shape[2] % heads:
        return f"q {tuple(q.shape)} does not split into {heads} heads"
    dh = q.shape[2] // heads
    if dh % 8 or not 8 <= dh <= 512:
        return f"head dim {dh} is not a multiple of 8 in 8 .. 512"
    return None


def attention_x3_ok(q: torch.Tensor, k: torch.Tensor, vt: torch.Tensor, heads: int, n_keys: int) -> bool:
    """True where `attention(..., flash=True)` is defined: fp32 tensors on the device, d_head a multiple of 8 up to 512."""
    return n_keys > 0 and _attention_x3_why_not(q, k, vt, heads) is None


def attention(q: torch.Tensor, k: torch.Tensor, vt: torch.Tensor, heads: int, n_keys: int, scale: float, flash: Optional[bool] = None) -> torch.Tensor:
    """softmax(Q K^T * scale) V with heads split along the channel dim.
    q: [B, Nq, C], k: [B, Nk, C], vt: [B, C, ld] (V transposed, ld = roundup(Nk, 8)) -> [B, Nq, C].
    k may hold more than n_keys rows per batch: the first n_keys of every batch are the keys (with several batches that costs a copy).
    Pad columns n_keys..ld of vt: the flash branch (half type, d_head <= 160) masks keys >= n_keys and never reads them unmasked, so
    anything may sit there.  The unfused branch (fp32, or d_head > 160) does NOT mask: its PV GEMM runs over roundup(n_keys, 8)
    columns and multiplies the pads by the score buffer's pad columns, which are exact zeros - finite pads drop out bitwise,
    non-finite ones (NaN, inf) would poison every output.  Every producer in this package (`linear_transposed`, `linear` /
    `ln_linear` with transposed_from) zeroes them; a caller that builds vt itself must do the same.
    flash (fp32 inputs only; half-type inputs ignore it): True = the fp32-class flash kernel (crg_attention_x3) or a CrgError naming
    the violated condition; False = the unfused branch; None = the flash kernel when knobs.ATTN_X3_FLASH is set and attention_x3_ok
    holds, else the unfused branch.  The flash kernel masks keys >= n_keys like the half-type one and needs only n_keys columns of vt."""
    if flash and q.dtype != HALF:
        why = _attention_x3_why_not(q, k, vt, heads)
        if why is not None:
            raise L.CrgError(f"attention(flash=True): {why}")
    _need_cuda(q, k, vt)
    if q.dim() != 3 or k.dim() != 3 or vt.dim() != 3:
        raise L.CrgError("attention: q [B, Nq, C], k [B, Nk, C] and vt [B, C, ld] expected")
    B, Nq, Cc = q.shape
    if heads <= 0 or Cc % heads:
        raise L.CrgError(f"attention: width {Cc} does not split into {heads} heads")
    if k.shape[0] != B or k.shape[2] != Cc or vt.shape[0] != B or vt.shape[1] != Cc:
        raise L.CrgError(f"attention: k {tuple(k.shape)} / vt {tuple(vt.shape)} do not match q {tuple(q.shape)} in batch and width")
    if k.dtype != q.dtype or vt.dtype != q.dtype:
        raise L.CrgError(f"attention: q, k and vt must share one dtype, got {q.dtype}, {k.dtype}, {vt.dtype}")
    if not 0 < n_keys <= min(k.shape[1], vt.shape[-1]):
        raise L.CrgError(f"attention: n_keys = {n_keys} outside k's {k.shape[1]} rows / vt's {vt.shape[-1]} columns")
    Dh = Cc // heads
    if q.dtype == torch.float32 and (flash if flash is not None else knobs.ATTN_X3_FLASH and attention_x3_ok(q, k, vt, heads, n_keys)):
        return _attention_x3(q, k, vt, heads, n_keys, scale)
    flash = q.dtype == HALF and Dh <= 160
    if not flash and vt.shape[-1] < (n_keys + 7) // 8 * 8:
        raise L.CrgError(f"attention: the unfused branch reads roundup(n_keys, 8) columns of vt, which has {vt.shape[-1]} for {n_keys} keys")
    vt = vt.contiguous()  # no-op for the [B, C, ld] every producer of this package returns; ld is taken as the row stride below
    ld = vt.shape[-1]
    if flash:
        # q / k may be column slices of one fused projection output: rows keep their parent stride.  The kernels step from batch to batch
        # by n_keys rows of k: a k buffer with more rows than n_keys is cut to them (and copied, unless there is one batch only)
        def rows(t):
            if t.stride(2) != 1 or (B > 1 and t.stride(0) != t.shape[1] * t.stride(1)):
                t = t.contiguous()
            return t, t.stride(1)
        q, ldq = rows(q)
        k, ldk = rows(k[:, :n_keys])
        o = torch.empty((B, Nq, Cc), dtype=q.dtype, device=q.device)
        _call("crg_attention", q, _p(q), ldq, _p(k), ldk, _p(vt), ld, _p(o), Cc, B, heads, Nq, n_keys, Dh, scale, L.BF16)
        return o
    q, k = q.contiguous(), k.contiguous()
    # Unfused path: S = QK^T (fp32) -> row softmax -> PV, all on the GEMM kernels.  Serves the fp32-class (BF16X3)
    # configuration and head dims beyond the flash kernel (the VAE's single-head C=512 AttnBlock, model.py:185-209).
    # The score matrix is never held whole: queries are processed in chunks sized so that the fp32 score buffer stays
    # <= knobs.SCORE_BUDGET_BYTES (the reference's original path materialises all of it - 1 GiB per image at 1024x1024,
    # attention.py:389-429), hi / lo planes come from crg_split_bf16, and no PyTorch arithmetic runs.
    split = q.dtype == torch.float32
    o = torch.empty_like(q)
    kp = (n_keys + 7) // 8 * 8
    prec = L.PREC_BF16X3 if split else L.PREC_BF16
    h = _h(q)

    def planes(t):
        if not split:
            return t, None
        th, tl = torch.empty(t.shape, dtype=HALF, device=t.device), torch.empty(t.shape, dtype=HALF, device=t.device)
        _call("crg_split_bf16", t, _p(t), _p(th), _p(tl), t.numel())
        return th, tl
    kh, kl = planes(k)            # [B, Nk, C]
    vh, vl = planes(vt)           # [B, C, ld]
    qc = max(8, min(Nq, knobs.SCORE_BUDGET_BYTES // (4 * heads * kp) // 8 * 8))  # queries per chunk
    s = torch.empty((heads, min(qc, Nq), kp), dtype=torch.float32, device=q.device)
    if kp != n_keys:
        s[:, :, n_keys:].zero_()
    for b in range(B):
        for q0 in range(0, Nq, qc):
            nq = min(qc, Nq - q0)
            sv = s[:, :nq]
            ld_s = s.shape[1] * kp  # head stride of the score buffer
            # (no bias, residual or activation: those fields of crg_gemm_args stay zero; both calls lie inside one sample)
            _gemm(h, a=q[b, q0:].data_ptr(), lda=Cc, a_bstride=Dh, w=kh[b].data_ptr(), w_lo=kl[b].data_ptr() if split else None, ldw=Cc, w_bstride=Dh,
                  y=sv.data_ptr(), ldy=kp, y_bstride=ld_s, M=nq, N=n_keys, K=Dh, batch=heads, a_dtype=_act_dt(q), y_dtype=L.F32, prec=prec, rows_per_sample=nq)
            if nq == s.shape[1]:
                softmax_rows_(s, n_keys, scale)
            else:  # last, shorter chunk: the rows of one head are contiguous [nq, kp]
                for hd in range(heads):
                    softmax_rows_(s[hd, :nq], n_keys, scale)
            _gemm(h, a=sv.data_ptr(), lda=kp, a_bstride=ld_s, w=vh[b].data_ptr(), w_lo=vl[b].data_ptr() if split else None, ldw=ld, w_bstride=Dh * ld,
                  y=o[b, q0:].data_ptr(), ldy=Cc, y_bstride=Dh, M=nq, N=Dh, K=kp, batch=heads, a_dtype=L.F32, y_dtype=_act_dt(q), prec=prec, rows_per_sample=nq)
    return o


def _attention_x3(q, k, vt, heads, n_keys, scale):
    """The fp32-class flash route of `attention` (arguments already checked there)."""
    B, Nq, Cc = q.shape
    k = k[:, :n_keys]

    def rows(t):  # column slices keep their parent's row stride; the kernel wants 16-byte aligned rows one batch stride apart
        if (t.stride(2) != 1 or t.stride(1) % 4 or t.stride(1) < Cc or t.data_ptr() % 16
                or (B > 1 and t.stride(0) != t.shape[1] * t.stride(1))):
            t = t.contiguous()
        return t, t.stride(1)
    q, ldq = rows(q)
    k, ldk = rows(k)
    vt = vt.contiguous()  # no-op for the [B, C, ld] every producer of this package returns
    o = torch.empty((B, Nq, Cc), dtype=torch.float32, device=q.device)
    a = L.AttnX3Args(q=q.data_ptr(), ldq=ldq, k=k.data_ptr(), ldk=ldk, vt=vt.data_ptr(), ldvt=vt.shape[-1], o=o.data_ptr(), ldo=Cc,
                     B=B, H=heads, Nq=Nq, Nk=n_keys, Dh=Cc // heads, scale=scale)
    _call("crg_attention_x3", q, C.byref(a))
    return o


def attention_rows_v(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, heads: int, scale: float) -> torch.Tensor:
    """softmax(Q K^T * scale) V with V ROW-MAJOR ([B, Nk, C], like K): q, k, v may be column slices of one fused projection
    output (rows keep the parent's stride), which is what makes `to_q | to_k | to_v` ONE GEMM launch.  bf16, d_head <= 160
    (crg_attention_v: the flash kernel transposes V on its LDS read)."""
    _need_cuda(q, k, v)
    B, Nq, Cc = q.shape
    Nk = k.shape[1]
    Dh = Cc // heads
    if q.dtype != HALF or Dh > 160 or k.shape != v.shape or k.shape[0] != B or k.shape[2] != Cc:
        raise L.CrgError("attention_rows_v: bf16 q / k / v with matching shapes and d_head <= 160 expected")

    def rows(t):
        if t.stride(2) != 1 or t.stride(0) != t.shape[1] * t.stride(1):
            t = t.contiguous()
        return t, t.stride(1)
    q, ldq = rows(q)
    k, ldk = rows(k)
    v, ldv = rows(v)
    o = torch.empty((B, Nq, Cc), dtype=q.dtype, device=q.device)
    _call("crg_attention_v", q, _p(q), ldq, _p(k), ldk, _p(v), ldv, _p(o), Cc, B, heads, Nq, Nk, Dh, scale, L.BF16)
    return o
