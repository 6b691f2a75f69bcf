"""The edges of the library's 16-bit type, in both builds: this file runs in the default process (bfloat16, libcrg_hip.so) and in
the child process of tests/test_hip_ops_f16.py (CRG_HALF=f16, libcrg_hip_f16.so); every case states what it expects per type.

  * fp32-class operands are carried as two half-type planes hi = half(x), lo = half(x - hi).  With fp16 planes lo is an fp16
    SUBNORMAL for every |x| below about 0.125: a conversion, an LDS-DMA path or a matrix instruction that flushed subnormals would
    cost the fp32-class ops three decimal digits (CPU emulation below) without any other test noticing.
  * fp16 ends at 65504: operands up to 3e4 and results below 6e4 must come out finite and at the type's accuracy.
  * the attention rounds P to the half type before P V: probabilities below 2^-14 are fp16 subnormals.
  * softmax shifts in the hundreds on the few-keys kernel.
  * LayerNorm statistics of rows with a common offset of 50 and 100 standard deviations (the epilogue route folds E[x^2] - mean^2).

References are plain fp64 PyTorch on the stored (already rounded) inputs.  Bounds: `check()` of tests/test_hip_ops.py (half-type bounds
scale with the type's unit round-off, HS; fp32-class bounds do not), or derived here from a CPU emulation of the arithmetic the
kernels state, never from the GPU's output.
"""
import os

import pytest
import torch
import torch.nn.functional as F

from tests.test_hip_ops import BF, HALF_F16, HS, _dev, check, fig, nhwc, q, rnd

pytestmark = pytest.mark.gpu

F32 = torch.float32


def test_library_of_this_process_half_type():
    """First of all: the process really runs the library of its half type (the fp16 child must not silently test libcrg_hip.so)."""
    from cremage_amd import _lib, ops
    assert _lib.HALF_F16 == HALF_F16 and ops.HALF == BF
    assert _lib.load().crg_half_kind() == (1 if HALF_F16 else 0)
    if not os.environ.get("CRG_LIB"):
        assert os.path.basename(_lib.LIB_PATH) == ("libcrg_hip_f16.so" if HALF_F16 else "libcrg_hip.so")
    y = ops.silu(torch.zeros(8, device=_dev(), dtype=BF))
    assert y.dtype == BF


# ------------------------------------------------------------------------------------------ fp32-class operands
def _planes(t, flush):
    """hi = half(t), lo = half(t - hi) (small_ops.hip split_bf16_kernel) as fp32; `flush`: plane values that are fp16 subnormals
    (|v| < 2^-14) become zero - what a flushing conversion or matrix instruction would see"""
    hi = t.to(BF).float()
    lo = (t - hi).to(BF).float()
    if flush:
        hi = torch.where(hi.abs() < 2.0 ** -14, torch.zeros_like(hi), hi)
        lo = torch.where(lo.abs() < 2.0 ** -14, torch.zeros_like(lo), lo)
    return hi, lo


def _three_pass(op, x, w, flush=False):
    """CPU emulation of the fp32-class product as gemm_reg_kernel.h states it: three matrix passes hi*hi + hi*lo + lo*hi on half-type
    planes (lo*lo dropped), fp32 accumulate, fp32 result.  `op(x, w)` is the bias-free linear map in the dtype of its arguments."""
    xh, xl = _planes(x, flush)
    wh, wl = _planes(w, flush)
    return op(xh, wh) + (op(xh, wl) + op(xl, wh))


def _rel(a, b):
    return ((a.double() - b.double()).norm() / b.double().norm().clamp_min(1e-30)).item()


def _fp32_class_bound(op, x, w, bias, small):
    """rel-L2 bound of an fp32-class op on these inputs.  Activations of order one: the suite's fp32-class bound (check(): 5e-5; the
    emulation gives ~5e-7 with fp16 subnormals kept and ~2e-4 with them flushed, so it separates the two).  Activations of scale 0.02
    next to a bias of scale one: the error of the product is 50x smaller against the output, so the bound comes from the emulation on
    these very inputs - fp16: the geometric mean of 'subnormals kept' and 'subnormals flushed'; bf16 (planes keep the fp32 exponent
    range, nothing to flush): twice the emulated error, for the summation order."""
    if not small:
        return 5e-5
    ref = op(x.double(), w.double()) + bias.double()
    kept = _rel(_three_pass(op, x, w) + bias, ref)
    if not HALF_F16:
        return 2.0 * kept
    flushed = _rel(_three_pass(op, x, w, flush=True) + bias, ref)
    assert flushed > 20 * kept, (kept, flushed)  # the inputs do separate the two behaviours
    return (kept * flushed) ** 0.5


def _act(shape, seed, small):
    return rnd(*shape, seed=seed, scale=0.02) if small else rnd(*shape, seed=seed, scale=2.0) + 0.5


def _judge(got, ref, bound, what):
    got, ref = got.double().cpu(), ref.double()
    assert got.shape == ref.shape and torch.isfinite(got).all(), what
    rel = fig(what + " rel-L2", _rel(got, ref), bound)
    mx = fig(what + " max-abs", (got - ref).abs().max().item(), ref.abs().max().item() * 1e-4 + 1e-5)
    assert rel < bound and mx < ref.abs().max().item() * 1e-4 + 1e-5, (what, rel, bound, mx)


def test_split_planes_reproduce_small_and_large_values():
    """crg_split_bf16 on magnitudes from 1e-5 to 10.  fp16 planes: hi + lo reproduces x to 2^-22 |x| while lo is a normal fp16 number and
    to 2^-25 (half the subnormal quantum 2^-24) below; bf16 planes: to 2^-16 |x| everywhere.  A flushed lo plane would be off by up to
    2^-15 for |x| < 0.125."""
    from cremage_amd import ops
    g = torch.Generator().manual_seed(700)
    mag = 10.0 ** (torch.rand(2, 64, 16, 16, generator=g) * 6.0 - 5.0)
    x = mag * torch.where(torch.rand(mag.shape, generator=g) < 0.5, -1.0, 1.0)
    xd = nhwc(x, F32)
    hi, lo = ops.split_bf16(xd)
    assert hi.dtype == lo.dtype == BF
    err = (hi.double() + lo.double() - xd.double()).abs().cpu()
    ax = x.double().abs()
    bound = torch.maximum(ax * 2.0 ** -22, torch.full_like(ax, 2.0 ** -25)) if HALF_F16 else ax * 2.0 ** -16
    fig("split planes: worst error / bound", (err / bound).max().item(), 1.0)
    assert (err <= bound).all()
    if HALF_F16:
        small = ax < 0.05
        assert (lo.float().cpu()[small].abs() < 2.0 ** -14).all() and (lo.float().cpu()[small] != 0).any()  # lo really is subnormal there


CONV_CASES = [  # (name, N, C, H, W, Co, ksize, operand form)
    ("staged3x3", 1, 128, 16, 20, 128, 3, "fp32"),     # fp32 tensor in, split while staging through registers
    ("planes3x3", 1, 128, 16, 20, 128, 3, "planes"),   # pre-split planes, width 20: the tap-wise LDS-DMA implicit GEMM
    ("planes1x1", 2, 128, 16, 20, 96, 1, "planes"),
    ("rowhalo", 1, 128, 16, 32, 128, 3, "planes"),     # width divides 128: conv3_rowhalo_kernel (the shape of the emulation table)
]


@pytest.mark.parametrize("small", [False, True], ids=["unit", "small"])
@pytest.mark.parametrize("case", CONV_CASES, ids=[c[0] for c in CONV_CASES])
def test_fp32_class_conv_small_magnitudes(case, small):
    """fp32-class convs whose operands put the lo plane (and, at scale 0.02, much of the hi plane's tail) into fp16's subnormal range."""
    from cremage_amd import ops
    _, N, C, H, W, Co, ks, form = case
    x = _act((N, C, H, W), 710, small)
    w, b = rnd(Co, C, ks, ks, seed=711, scale=(C * ks * ks) ** -0.5), rnd(Co, seed=712)
    op = lambda a, ww: F.conv2d(a, ww, None, padding=ks // 2)
    bound = _fp32_class_bound(op, x, w, b[None, :, None, None], small)
    ref = op(x.double(), w.double()) + b.double()[None, :, None, None]
    xd = nhwc(x, F32)
    if form == "fp32":
        got = ops.conv2d(xd, w.to(_dev()), b.to(_dev()), padding=ks // 2)
    else:
        hi, lo = ops.split_bf16(xd)
        got = ops.conv2d(hi, w.to(_dev()), b.to(_dev()), x_lo=lo, padding=ks // 2)
    assert got.dtype == F32
    _judge(got, ref, bound, f"fp32-class conv {case[0]} {'0.02' if small else 'unit'}")


@pytest.mark.parametrize("small", [False, True], ids=["unit", "small"])
def test_fp32_class_linear_small_magnitudes(small):
    from cremage_amd import ops
    M, K, N = 256, 640, 320
    x, w, b = _act((M, K), 720, small), rnd(N, K, seed=721, scale=K ** -0.5), rnd(N, seed=722)
    op = lambda a, ww: F.linear(a, ww)
    bound = _fp32_class_bound(op, x, w, b, small)
    got = ops.linear(x.to(_dev()), w.to(_dev()), b.to(_dev()))
    assert got.dtype == F32
    _judge(got, op(x.double(), w.double()) + b.double(), bound, f"fp32-class linear {'0.02' if small else 'unit'}")


@pytest.mark.parametrize("small", [False, True], ids=["unit", "small"])
def test_group_norm_split_feeds_fp32_class_conv(small):
    """crg_groupnorm_split -> planes -> row-halo conv, as the VAE chains them; `small`: gamma of scale 0.02, so that the normalised
    activations (and both planes) are small.  Against fp64 GroupNorm + SiLU + conv; the GroupNorm itself is fp32 arithmetic (1e-6)."""
    from cremage_amd import ops
    N, C, H, W, Co = 1, 128, 16, 32, 128
    x = rnd(N, C, H, W, seed=730, scale=2.0) + 0.5
    s = 0.02 if small else 1.0
    g, be = s * (1 + 0.1 * rnd(C, seed=731)), s * 0.1 * rnd(C, seed=732)
    w, b = rnd(Co, C, 3, 3, seed=733, scale=(9 * C) ** -0.5), rnd(Co, seed=734)
    a64 = F.silu(F.group_norm(x.double(), 32, g.double(), be.double(), 1e-6))
    op = lambda a, ww: F.conv2d(a, ww, None, padding=1)
    bound = _fp32_class_bound(op, a64.float(), w, b[None, :, None, None], small)
    if small:
        bound = bound + 2e-8  # + the fp32 GroupNorm in front: 1e-6 relative on a term that is 0.02 of the output
    gh, gl = ops.group_norm(nhwc(x, F32), g.to(_dev()), be.to(_dev()), 32, 1e-6, silu=True, split=True)
    assert gh.dtype == gl.dtype == BF
    pl = (gh.double() + gl.double()).cpu()
    fig("GroupNorm planes vs fp64", (pl - a64).abs().max().item(), 1e-4 * s)
    assert (pl - a64).abs().max().item() < 1e-4 * s
    got = ops.conv2d(gh, w.to(_dev()), b.to(_dev()), x_lo=gl)
    _judge(got, op(a64, w.double()) + b.double()[None, :, None, None], bound, f"GroupNorm planes -> conv {'0.02' if small else 'unit'}")


# ------------------------------------------------------------------------------------------ top of the range
def _big(shape, seed):
    """activations of scale 1e4, clamped to |x| <= 3e4 (fp16 ends at 65504; the library's stated range)"""
    return (rnd(*shape, seed=seed) * 1e4).clamp(-3e4, 3e4)


@pytest.mark.parametrize("form", ["fp32", "planes", "half"])
@pytest.mark.parametrize("W", [20, 32])  # the tap-wise implicit GEMM / the row-halo kernel
def test_conv_top_of_range(form, W):
    """|x| up to 3e4, weights scaled so that the outputs stay below 6e4: finite, and at the accuracy of order-one operands."""
    from cremage_amd import ops
    N, C, H, Co = 1, 128, 16, 128
    x = _big((N, C, H, W), 740)
    w, b = rnd(Co, C, 3, 3, seed=741, scale=0.5 * (9 * C) ** -0.5), rnd(Co, seed=742)
    dt = BF if form == "half" else F32
    ref = F.conv2d(q(x, dt).double(), (q(w, BF) if form == "half" else w).double(), b.double(), padding=1)
    assert 1e4 < ref.abs().max().item() < 6e4
    if form == "planes":
        hi, lo = ops.split_bf16(nhwc(x, F32))
        got = ops.conv2d(hi, w.to(_dev()), b.to(_dev()), x_lo=lo)
    else:
        got = ops.conv2d(nhwc(x, dt), w.to(_dev()), b.to(_dev()))
    check(got, ref, dt, f"conv top of range {form} W={W}")


@pytest.mark.parametrize("dtype", [BF, F32], ids=["half", "fp32"])
def test_linear_top_of_range(dtype):
    from cremage_amd import ops
    M, K, N = 256, 640, 320
    x, w, b = _big((M, K), 750), rnd(N, K, seed=751, scale=0.5 * K ** -0.5), rnd(N, seed=752)
    ref = F.linear(q(x, dtype).double(), (q(w, BF) if dtype == BF else w).double(), b.double())
    assert 1e4 < ref.abs().max().item() < 6e4
    check(ops.linear(x.to(_dev()).to(dtype), w.to(_dev()), b.to(_dev())), ref, dtype, "linear top of range")


@pytest.mark.parametrize("dtype", [BF, F32], ids=["half", "fp32"])
@pytest.mark.parametrize("C,hw", [(128, 16), (320, 64)])  # the single-launch path / the statistics + apply pair
def test_group_norm_top_of_range(dtype, C, hw):
    """x of scale 1e4 around 5e3: x^2 is far beyond fp16; statistics are fp32 and shifted, the output is of order one."""
    from cremage_amd import ops
    x = (rnd(2, C, hw, hw, seed=760) * 8e3 + 5e3).clamp(-3e4, 3e4)
    g, b = 1 + 0.1 * rnd(C, seed=761), 0.1 * rnd(C, seed=762)
    ref = F.silu(F.group_norm(q(x, dtype).double(), 32, g.double(), b.double(), 1e-5))
    got = ops.group_norm(nhwc(x, dtype), g.to(_dev()), b.to(_dev()), 32, 1e-5, silu=True)
    check(got, ref, dtype, "group_norm top of range")


# ------------------------------------------------------------------------------------------ attention
def _heads(t, heads):
    B, n, C = t.shape
    return t.reshape(B, n, heads, C // heads).permute(0, 2, 1, 3)


@pytest.mark.parametrize("heads,d,Nq,Nk,entry", [
    (2, 40, 200, 2048, "vt"),    # software-pipelined kernel (Nk % 128 == 0), shift inside the MFMA
    (2, 80, 200, 2048, "vt"),    # software-pipelined kernel, d 80
    (2, 64, 200, 2048, "vt"),    # d 64: the plain LDS-DMA kernel (attention.hip dispatch)
    (2, 40, 200, 1984, "vt"),    # 31 key tiles: odd tile count, the plain LDS-DMA kernel
    (2, 48, 200, 2048, "vt"),    # register-staged kernel
    (2, 40, 200, 2048, "rows"),  # row-major V entry (crg_attention_v)
])
def test_attention_crowd_of_improbable_keys(heads, d, Nq, Nk, entry):
    """One dominant key inside the first key tile, then a crowd of Nk - 1 keys whose logits lie about 16 log2 units below it: each
    crowd probability (~2^-16, against P = 1 for the dominant key the first tile sets the reference to) is an fp16 SUBNORMAL once P is
    rounded to the half type for P V, and together the crowd carries 3 % of the softmax mass.  V is +1 on the crowd and -1 on the dominant
    key, so a flushed crowd moves every output element by 6 %.  Judged per query row and head.  CPU emulation on these inputs with P
    (relative to the first tile's maximum) and the output rounded to the half type, fp64 elsewhere: worst row 2.2e-4 in fp16 with
    subnormals kept, 4.8e-2 with P flushed, 2.1e-3 in bf16; bound: the half type's attention bound of tests/test_hip_ops.py (1e-2 * HS)."""
    from cremage_amd import ops
    B, C, scale = 2, heads * d, d ** -0.5
    g = torch.Generator().manual_seed(770 + d)
    e = torch.where(torch.rand(heads, d, generator=g) < 0.5, -1.0, 1.0) * d ** -0.5          # a unit direction per head
    a = (16.0 * 0.6931471805599453 / scale) ** 0.5                                           # scale * a * a = 16 log2 units
    qq = (a * e[None, None] + 0.06 * torch.randn(B, Nq, heads, d, generator=g)).reshape(B, Nq, C)
    kk = (0.1 / (scale * a)) * torch.randn(B, Nk, heads, d, generator=g)                      # crowd: logits of +-0.1 nats around zero
    kk[:, 5] = a * e[None]                                                                   # the dominant key
    kk = kk.reshape(B, Nk, C)
    vv = 1.0 + 0.5 * torch.randn(B, Nk, C, generator=g)
    vv[:, 5] = -1.0 + 0.05 * torch.randn(B, C, generator=g)
    q64, k64, v64 = (_heads(q(t, BF).double(), heads) for t in (qq, kk, vv))
    p = torch.softmax(q64 @ k64.transpose(-1, -2) * scale, dim=-1)
    crowd = torch.cat([p[..., :5], p[..., 6:]], dim=-1)
    assert (crowd / p[..., 5:6]).max().item() < 2.0 ** -14.3, "a crowd key is not in fp16's subnormal range"
    assert 0.02 < crowd.sum(-1).min().item() and crowd.sum(-1).max().item() < 0.045
    ref = p @ v64                                                                            # [B, heads, Nq, d]
    dq, dk = qq.to(_dev()).to(BF), kk.to(_dev()).to(BF)
    if entry == "rows":
        got = ops.attention_rows_v(dq, dk, vv.to(_dev()).to(BF), heads, scale)
    else:
        got = ops.attention(dq, dk, vv.transpose(1, 2).contiguous().to(_dev()).to(BF), heads, Nk, scale)
    got = _heads(got.double().cpu(), heads)
    assert torch.isfinite(got).all()
    rows = ((got - ref).norm(dim=-1) / ref.norm(dim=-1))
    worst = fig(f"attention crowd d{d} Nk{Nk} {entry}: worst row", rows.max().item(), 1e-2 * HS)
    rel = fig(f"attention crowd d{d} Nk{Nk} {entry}: rel-L2", _rel(got, ref), 1e-2 * HS)
    assert worst < 1e-2 * HS and rel < 1e-2 * HS, (worst, rel)


@pytest.mark.parametrize("row_major_v", [False, True])
def test_few_keys_kernel_large_logits(row_major_v):
    """attn_ctx_kernel (Nk = 77, B = 16: the dispatch of test_flash_attention_few_keys_kernel) with a gain of 30 on Q: logits in the
    hundreds, a near-one-hot softmax, negative row maxima.  Bound: that of test_flash_attention_large_logits at this gain (the same
    statement - a near-one-hot softmax amplifies the half-type rounding of Q * scale * log2(e), and the winner can change between two
    close keys), 2e-2 * HS."""
    from cremage_amd import ops
    B, heads, d, Nq, Nk = 16, 8, 40, 2100, 77
    assert (Nq + 127) // 128 * B * heads >= 2048 and Nk <= 128  # the dispatch rule of attention_entry (attention.hip)
    C = heads * d
    qq, kk, vv = rnd(B, Nq, C, seed=780) * 30.0, rnd(B, Nk, C, seed=781), rnd(B, Nk, C, seed=782)
    kk[:, 40:] *= 3.0                # larger logits in the second key tile
    qq[:, :16] = -qq[:, :16].abs()   # rows whose logits against the positive keys below are all negative
    kk[:, :8] = kk[:, :8].abs()
    q64, k64, v64 = (_heads(q(t, BF).double(), heads) for t in (qq, kk, vv))
    ref = torch.softmax(q64 @ k64.transpose(-1, -2) * d ** -0.5, dim=-1) @ v64
    dq, dk = qq.to(_dev()).to(BF), kk.to(_dev()).to(BF)
    if row_major_v:
        got = ops.attention_rows_v(dq, dk, vv.to(_dev()).to(BF), heads, d ** -0.5)
    else:
        vt = torch.full((B, C, (Nk + 7) // 8 * 8), float("nan"))
        vt[:, :, :Nk] = vv.transpose(1, 2)
        got = ops.attention(dq, dk, vt.to(_dev()).to(BF), heads, Nk, d ** -0.5)
    got = _heads(got.double().cpu(), heads)
    assert torch.isfinite(got).all()
    rel = fig("few-keys attention, gain 30: rel-L2", _rel(got, ref), 2e-2 * HS)
    assert rel < 2e-2 * HS, rel


# ------------------------------------------------------------------------------------------ LayerNorm with a large common offset
def _offset_rows(B, T, K, ratio):
    """LayerNorm input as `to_out + residual` writes it (a GEMM of this library, with row statistics), every row around a common
    offset of `ratio` standard deviations (the rows have variance 2: unit GEMM output + unit residual)"""
    from cremage_amd import ops
    dev = _dev()
    x0, w0 = rnd(B, T, K, seed=790), rnd(K, K, seed=791, scale=K ** -0.5)
    r0 = rnd(B, T, K, seed=792) + ratio * 2.0 ** 0.5
    return ops.linear(x0.to(dev).to(BF), w0.to(dev), residual=r0.to(dev).to(BF), row_stats=True)


@pytest.mark.parametrize("ratio", [50.0, 100.0])
@pytest.mark.parametrize("M,K,N,act,vt", [(512, 640, 640, None, False), (512, 640, 1920, None, True), (512, 640, 5120, "geglu", False),
                                          (512, 1280, 1280, None, False), (512, 1280, 3840, None, True), (512, 1280, 10240, "geglu", False),
                                          (8192, 640, 5120, "geglu", False)])  # last: 5 tiles per CU, the persistent ring kernel's fold
def test_layernorm_epilogue_large_offset(M, K, N, act, vt, ratio):
    """The LayerNorm-as-epilogue route takes the variance as E[x^2] - mean^2 from the producer's fp32 row partials and corrects with
    mean * colsum (gemm_shared.h ln_row_coeffs): rows whose mean is 50 and 100 standard deviations.  A CPU emulation of that single-pass
    formula in fp32 (M = 512, K = 640) stays inside check()'s half-type bound at both ratios (fp16, offset 100: plain rel-L2 3.6e-4,
    GEGLU 5.6e-4 against 7.5e-4; bf16: 1.7e-3 against 6e-3), so these are inputs the formula itself passes.  Against fp64 LayerNorm +
    Linear on the stored rows with W o gamma rounded once.
    Measured on MI355X, fp16, offset 100: with the fold, 1 / K and mean^2 in fp32 the kernels gave plain 5.7e-4 and GEGLU 9.8e-4 (over the
    bound); with the fold in fp64 (as it is now) plain 4.2e-4, GEGLU 7.0e-4.  What remains above the 2.1e-4 of the output rounding is
    the rounding of the producer's fp32 partial sums of squares (80 columns each, ~1.6e6 at this offset)."""
    from cremage_amd import ops
    dev = _dev()
    T = 256
    B = M // T
    x = _offset_rows(B, T, K, ratio)
    assert getattr(x, "_crg_ln", None) is not None
    g, be = 1.0 + 0.3 * rnd(K, seed=793), 0.2 * rnd(K, seed=794)
    w, b = rnd(N, K, seed=795, scale=K ** -0.5), rnd(N, seed=796)
    ln = torch.nn.LayerNorm(K).to(dev)
    with torch.no_grad():
        ln.weight.copy_(g)
        ln.bias.copy_(be)
    assert ops.ln_epi_ok(x, w.to(dev), act)
    xr = x.double().cpu()
    assert abs(xr.mean().item() / xr.std(dim=-1).mean().item() - ratio) < 0.1 * ratio
    xhat = F.layer_norm(xr, (K,), None, None, ln.eps)
    ref = F.linear(xhat, q(w * g, BF).double(), (w.double() @ be.double()) + b.double())
    if act == "geglu":
        ref = ref[..., :N // 2] * F.gelu(ref[..., N // 2:])
    n0 = 2 * (N // 3) if vt else None
    got = ops.linear(x, w.to(dev), b.to(dev), act=act, transposed_from=n0, ln=(ln.weight, ln.bias, ln.eps))
    if vt:
        qk, vt_ = got
        assert (vt_[:, :, T:] == 0).all()
        got = torch.cat([qk, vt_[:, :, :T].transpose(1, 2)], dim=-1)
    check(got, ref, BF, f"LN epilogue, offset {ratio:g} sigma, {M}x{K}->{N} {act}")


@pytest.mark.parametrize("ratio", [50.0, 100.0])
def test_layernorm_two_pass_large_offset(ratio):
    """The same rows through the two-pass kernels: crg_ln_gemm (K = 320; the MFMA operand is LN(x) rounded to the half type once, as
    test_ln_linear states) and the stand-alone crg_layernorm (K = 320, 640, 1280)."""
    from cremage_amd import ops
    dev = _dev()
    for K in (320, 640, 1280):
        x = _offset_rows(2, 256, K, ratio)
        xr = x.double().cpu()
        g, be = 1.0 + 0.3 * rnd(K, seed=797), 0.2 * rnd(K, seed=798)
        ln64 = F.layer_norm(xr, (K,), g.double(), be.double(), 1e-5)
        check(ops.layer_norm(x, g.to(dev), be.to(dev), 1e-5), ln64, BF, f"layer_norm, offset {ratio:g} sigma, K={K}")
        if K == 320:
            N = 960
            w, b = rnd(N, K, seed=799, scale=K ** -0.5), rnd(N, seed=800)
            dw = w.to(dev).to(BF)
            assert ops.ln_linear_ok(x, dw)
            ref = F.linear(q(ln64, BF).double(), q(w, BF).double(), b.double())
            check(ops.ln_linear(x, g.to(dev), be.to(dev), 1e-5, dw, b.to(dev)), ref, BF, f"ln_linear, offset {ratio:g} sigma")
