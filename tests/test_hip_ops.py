"""Per-kernel parity on a real MI355X: every C-ABI entry point (through cremage_amd.ops -> ctypes ->
libcrg_hip.so) against a plain PyTorch fp32 CPU evaluation of the same op on the same seeded inputs.

Tolerances (stated per dtype):
  bf16 kernels     : inputs are rounded to bf16 first and the reference is evaluated on those rounded
                     values in fp32, so the remaining error is fp32-accumulate order + one bf16 output
                     rounding: rel-L2 <= 6e-3, max-abs <= 2^-7 * max|ref| (+ small abs floor).
  fp32-class (x3)  : split-bf16 operands carry ~2^-17 relative error each: rel-L2 <= 5e-5.

The half type is the process's (CRG_HALF, as cremage_amd/_lib.py reads it): `BF` below is "the library's 16-bit type", bfloat16 by
default and IEEE fp16 under CRG_HALF=f16 (tests/test_hip_ops_f16.py runs this file in such a child process against
libcrg_hip_f16.so).  Every bound that is a statement about half-type round-off is written as <the bf16 figure> * HS, with HS the
type's unit round-off relative to bf16's (2^-9 -> 1, fp16's 2^-12 -> 1/8).  fp32-class bounds, statistics bounds, bitwise and shape
assertions do not depend on the half type.
"""
import math
import os

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

HALF_F16 = os.environ.get("CRG_HALF", "bf16").lower() in ("f16", "fp16", "float16", "half")  # cremage_amd/_lib.py:13 (no GPU call here)
BF = torch.float16 if HALF_F16 else torch.bfloat16  # the library's half type ("bf16" in the names below means this type)
HS = 2.0 ** -3 if HALF_F16 else 1.0                 # unit round-off of the half type over bf16's: the ONE factor on half-type bounds


def _dev():
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    return torch.device("cuda:0")


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


def fig(what, value, bound):
    """print a measured figure next to its bound (pytest -rP shows it for passing tests too: the headroom tables of the fp16 run)"""
    print(f"[fig] {what}: {value:.3e} (bound {bound:.3e})")
    return value


def check(got, ref, dtype, what=""):
    got = got.detach().float().cpu()
    ref = ref.detach().float().cpu()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert torch.isfinite(got).all(), what
    rel = ((got - ref).norm() / ref.norm().clamp_min(1e-20)).item()
    mx = (got - ref).abs().max().item()
    scale = ref.abs().max().item()
    fig(what + " rel-L2", rel, 6e-3 * HS if dtype == BF else 5e-5)
    fig(what + " max-abs", mx, (scale * 2 ** -6 + 1e-3) * HS if dtype == BF else scale * 1e-4 + 1e-5)
    if dtype == BF:
        assert rel < 6e-3 * HS and mx < (scale * 2 ** -6 + 1e-3) * HS, (what, rel, mx, scale)
    else:
        assert rel < 5e-5 and mx < scale * 1e-4 + 1e-5, (what, rel, mx, scale)


def q(x, dtype):
    """round to the kernel's storage dtype and come back to fp32 (reference sees what the kernel sees)"""
    return x.to(dtype).float()


def nhwc(x, dtype):
    return x.to(_dev()).to(dtype).contiguous(memory_format=torch.channels_last)


DTYPES = [BF, torch.float32]


def assert_route(what, **want):
    """which kernel the last crg_gemm / crg_conv2d call ran (ops.last_route(): the dispatcher's own record, crg_last_route), held against
    the route the case is about - a retuned threshold that moves a shape to another kernel fails here instead of passing on it"""
    from cremage_amd import ops
    r = ops.last_route()
    print(f"[route] {what}: " + " ".join(f"{k}={v}" for k, v in r.items()))
    assert {k: r[k] for k in want} == want, (what, r)


# ------------------------------------------------------------------------------------------ GEMM
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("M,N,K", [(128, 160, 64), (300, 320, 328), (77, 128, 768), (8, 1280, 320), (1000, 200, 72), (130, 36, 40),
                                   # one shape per tile configuration of the LDS-DMA kernel (gemm_glds_kernel.h; chosen by gemm_plan.h):
                                   (3000, 1280, 320),   # 192 tiles, short K          -> D (64-row tiles, 4 waves)
                                   (8200, 1280, 136),   # 520 tiles                   -> A (4 waves, 2 blocks per CU)
                                   (2048, 640, 1280),   # 64 tiles, short K           -> C (64-row tiles, 8 waves)
                                   (520, 320, 4096),    # 10 tiles, long K            -> A + split-K
                                   (35840, 320, 1024)]) # 560 tiles = 512 + 48        -> A + tail split (48 tiles cut along K)
def test_linear_shapes(dtype, M, N, K):
    from cremage_amd import ops
    x, w, b, r = rnd(M, K, seed=1), rnd(N, K, seed=2, scale=K ** -0.5), rnd(N, seed=3), rnd(M, N, seed=4)
    ref = F.linear(q(x, dtype), q(w, BF) if dtype == BF else w, b) + q(r, dtype)
    # half type: the LDS-DMA kernel in the configuration the shape's comment names (the unnamed small shapes: C); fp32: the register-staged
    # kernel, which has one configuration, cuts K by the same rule and has no tail split
    want = {(3000, 1280, 320): dict(config=4, splits=1), (8200, 1280, 136): dict(config=1, splits=1, tail_splits=0),
            (2048, 640, 1280): dict(config=3, splits=1), (520, 320, 4096): dict(config=1, splits=8, reduce="plain"),
            (35840, 320, 1024): dict(config=1, splits=1, tail_splits=4, reduce="plain")}.get((M, N, K), dict(config=3, splits=1, reduce="none"))
    if dtype == BF:
        want = dict(want, kernel="glds")
    else:
        want = dict(kernel="gemm_reg", config=0, splits=want["splits"], tail_splits=0)
    got = ops.linear(x.to(_dev()).to(dtype), w.to(_dev()), b.to(_dev()), residual=r.to(_dev()).to(dtype))
    assert_route(f"linear {M}x{N}x{K}", **want)
    check(got, ref, dtype, f"linear {M}x{N}x{K}")
    ref2 = F.silu(F.linear(q(x, dtype), q(w, BF) if dtype == BF else w, b))
    got2 = ops.linear(x.to(_dev()).to(dtype), w.to(_dev()), b.to(_dev()), act="silu")
    assert_route(f"linear+silu {M}x{N}x{K}", **want)
    check(got2, ref2, dtype, "linear+silu")


@pytest.mark.parametrize("B,T,K,C", [(8, 1024, 640, 640), (2, 256, 1280, 1280), (3, 1000, 320, 320), (4, 4096, 640, 640), (2, 64, 1280, 1280),
                                     # 65 x 24 = 1560 tiles = 3 x 512 + 24: the grid shape whose last 24 tiles used to go out as a K-split tail
                                     # launch, which cannot emit the transposed range (CrgError -22 mid-call)
                                     (10, 832, 1280, 1280)])
def test_linear_transposed_range(B, T, K, C):
    """crg_gemm with a transposed column range (the V third of a fused Q | K | V projection written as V^T [B][C][roundup(T, 8)] by the
    GEMM's own epilogue) on the three tile configurations (A / C / D), a token count that is no multiple of 8, and a K = 320 input
    that would otherwise take the LayerNorm-fused kernel."""
    from cremage_amd import ops
    dev = _dev()
    x, w = rnd(B, T, K, seed=310), rnd(3 * C, K, seed=311, scale=K ** -0.5)
    assert ops.linear_transposed_ok(x.to(dev).to(BF), w.to(dev), 2 * C)
    qk, vt = ops.linear(x.to(dev).to(BF), w.to(dev), transposed_from=2 * C)
    ref = F.linear(q(x, BF), q(w, BF))
    assert qk.shape == (B, T, 2 * C) and vt.shape == (B, C, (T + 7) // 8 * 8)
    check(qk, ref[..., :2 * C], BF, "q | k")
    check(vt[:, :, :T].transpose(1, 2), ref[..., 2 * C:], BF, "v transposed")
    assert (vt[:, :, T:] == 0).all()
    whole = ops.linear(x.to(dev).to(BF), w.to(dev))
    if (B * T + 127) // 128 * (3 * C // 160) % 512 in range(1, 225) and (B * T + 127) // 128 * (3 * C // 160) > 512:
        # without the transposed range this grid takes the K-split tail (another summation order for its last rows): close, not bitwise
        check(whole[..., :2 * C], qk.float(), BF, "q | k vs the untransposed launch")
        check(whole[..., 2 * C:], vt[:, :, :T].transpose(1, 2).float(), BF, "v vs the untransposed launch")
    else:
        assert torch.equal(whole[..., :2 * C], qk) and torch.equal(whole[..., 2 * C:], vt[:, :, :T].transpose(1, 2))


@pytest.mark.parametrize("M,N,K,res", [(8192, 640, 640, True),      # 256 tiles of 128 rows -> 64-row tiles (D)
                                       (32768, 320, 320, True),     # 512 tiles -> A, two blocks per CU
                                       (2048, 1280, 1280, True),    # 128 tiles -> C (8 waves, in-block split-K)
                                       (520, 1280, 1280, False),    # ragged M, C
                                       (4096, 1280, 5120, True),    # SDXL net[2] at the 32x32 level: 256 tiles, K = 80 k-tiles -> split-K, statistics from the reduce
                                       (1000, 648, 136, False)])    # N no multiple of the tile: a partial last n-tile
def test_row_stats_side_channel(M, N, K, res):
    """crg_gemm_args.row_stats: per row and column partial the sum / sum of squares of the ROUNDED outputs (the LayerNorm statistics
    the consuming GEMM folds), from the paired epilogue of every tile configuration and from the split-K reduce; the output itself is
    bitwise what the launch without the side channel writes."""
    from cremage_amd import ops
    dev = _dev()
    x, w, b, r = rnd(M, K, seed=41), rnd(N, K, seed=42, scale=K ** -0.5), rnd(N, seed=43), rnd(M, N, seed=44)
    args = (x.to(dev).to(BF), w.to(dev), b.to(dev))
    kw = dict(residual=r.to(dev).to(BF)) if res else {}
    y = ops.linear(*args, row_stats=True, **kw)
    y0 = ops.linear(*args, **kw)
    assert torch.equal(y, y0)
    st = getattr(y, "_crg_ln", None)
    assert st is not None and st[1] == y._version and st[0].shape == (M, ops.row_stats_parts(N), 2)
    s = st[0].double().sum(1).cpu()
    yf = y.double().cpu()
    assert (s[:, 0] - yf.sum(1)).abs().max().item() < 1e-4 * max(1.0, yf.abs().sum(1).max().item())
    assert (s[:, 1] - (yf * yf).sum(1)).abs().max().item() < 1e-4 * (yf * yf).sum(1).max().item()
    ops.axpby_(y, y0, 1.0, 1.0)  # a raw in-place write drops the side channel
    assert getattr(y, "_crg_ln", None) is None


@pytest.mark.parametrize("M,K,N,act,vt", [(8192, 640, 1920, None, True),      # Q | K | V of the 32x32 level, V third transposed (A)
                                          (8192, 640, 640, None, False),      # to_q of the cross-attention (D)
                                          (2048, 1280, 3840, None, True),     # 16x16 level (C)
                                          (512, 1280, 1280, None, False),     # 8x8 level (C), few rows
                                          (8192, 640, 5120, "geglu", False),  # GEGLU, 5 tiles per CU: the persistent ring kernel
                                          (2048, 1280, 10240, "geglu", False),  # GEGLU, 2.5 tiles per CU: the LDS-DMA kernel (unpaired epilogue)
                                          (4096, 1280, 3840, None, True),     # SDXL 32x32 level
                                          (32768, 320, 960, None, True),      # K = 320 on the epilogue route (CRG_LN_EPI_320 = 2)
                                          (32768, 320, 2560, "geglu", False)])
def test_layernorm_as_gemm_epilogue(M, K, N, act, vt, monkeypatch):
    """nn.LayerNorm + Linear (attention.py:900-912) as ONE GEMM on the raw rows: the producer of x (a GEMM + residual of this library)
    hands over row statistics, the consumer multiplies x by W o gamma and corrects in its epilogue (crg_gemm_args.ln_stats).  Against
    LayerNorm in fp32 on the very bf16 rows the producer stored; rows with a mean of six standard deviations exercise the
    cancellation mean * colsum; transposed V range, GEGLU (both kernels), every tile configuration."""
    from cremage_amd import ops
    monkeypatch.setattr(ops.knobs, "LN_EPI_320", 2)
    dev = _dev()
    mean = 0.0 if (M, N) in ((8192, 640), (512, 1280)) else 6.0  # (row means of six standard deviations: the cancellation mean * colsum)
    T = 1024 if M % 1024 == 0 else M
    B = M // T
    x0, w0, r0 = rnd(B, T, K, seed=51), rnd(K, K, seed=52, scale=K ** -0.5), rnd(B, T, K, seed=53) + mean
    x = ops.linear(x0.to(dev).to(BF), w0.to(dev), residual=r0.to(dev).to(BF), row_stats=True)  # the LayerNorm input, as to_out + residual writes it
    assert getattr(x, "_crg_ln", None) is not None
    g, be = 1.0 + 0.3 * rnd(K, seed=54), 0.2 * rnd(K, seed=55)
    w, b = rnd(N, K, seed=56, scale=K ** -0.5), rnd(N, seed=57)
    ln = torch.nn.LayerNorm(K).to(dev)
    with torch.no_grad():
        ln.weight.copy_(g)
        ln.bias.copy_(be)
    assert ops.ln_epi_ok(x, w.to(dev), act)
    xr = x.float().cpu()
    xhat = F.layer_norm(xr, (K,), None, None, ln.eps)
    ref = F.linear(xhat, q(w * g, BF), w @ be + b)       # the function the kernel evaluates (W o gamma rounded once)
    ref_plain = F.linear(F.layer_norm(xr, (K,), g, be, ln.eps), w, b)  # nn.LayerNorm + nn.Linear in fp32
    if act == "geglu":
        ref = ref[..., :N // 2] * F.gelu(ref[..., N // 2:])
        ref_plain = ref_plain[..., :N // 2] * F.gelu(ref_plain[..., N // 2:])
    n0 = 2 * (N // 3) if vt else None
    got = ops.ln_linear_auto(x, ln, w.to(dev), b.to(dev), act=act, transposed_from=n0)
    if vt:
        qk, vt_ = got
        got = torch.cat([qk, vt_[:, :, :T].transpose(1, 2)], dim=-1)
    check(got, ref, BF, f"LN epilogue {M}x{N}x{K} {act}")
    rel = ((got.float().cpu() - ref_plain).norm() / ref_plain.norm()).item()
    assert rel < 8e-3 * HS, rel  # vs fp32 LayerNorm + Linear: bf16 rounding of W o gamma and of the output


def test_linear_ring_gemm():
    """The persistent 256-row ring GEMM (gemm_ring.hip) against PyTorch in a child process that routes EVERY eligible shape to it
    (CRG_GEMM_RING=2, CRG_GEMM_RING_MIN=50: the knobs are read once per process; the default rule only takes GEGLU GEMMs with >= 3
    tiles per CU): several tiles per block (the ring runs across tile boundaries), ragged M (rows past M come from the descriptor's
    range check, their stores are dropped), an N that is no multiple of the tile width, residual / bias / GEGLU epilogues, both tile
    widths; the GEGLU call is bitwise reproducible."""
    import json
    import os
    import subprocess
    import sys
    from tests.conftest import REPO
    env = dict(os.environ, CRG_GEMM_RING="2", CRG_GEMM_RING_MIN="50")
    r = subprocess.run([sys.executable, os.path.join(REPO, "tests", "_ring_gemm_run.py")], env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    res = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RING_GEMM_RESULT ")][-1][len("RING_GEMM_RESULT "):])
    assert len(res) == 8
    for k, (rel, mx, scale, same) in res.items():
        assert rel < 6e-3 * HS and mx < (scale * 2 ** -6 + 1e-3) * HS and same, (k, rel, mx, scale, same)


@pytest.mark.parametrize("dtype", DTYPES)
def test_linear_batched_tokens_and_f32_out(dtype):
    from cremage_amd import ops
    x, w = rnd(2, 50, 96, seed=5), rnd(128, 96, seed=6, scale=0.1)
    ref = F.linear(q(x, dtype), q(w, BF) if dtype == BF else w)
    got = ops.linear(x.to(_dev()).to(dtype), w.to(_dev()), out_dtype=torch.float32)
    assert got.dtype == torch.float32 and got.shape == (2, 50, 128)
    check(got, ref, torch.float32 if dtype != BF else BF, "linear f32 out")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("M,C", [(60, 64), (257, 320)])
def test_geglu(dtype, M, C):
    from cremage_amd import ops
    x, w, b = rnd(M, C, seed=7), rnd(8 * C, C, seed=8, scale=C ** -0.5), rnd(8 * C, seed=9, scale=0.1)
    o = F.linear(q(x, dtype), q(w, BF) if dtype == BF else w, b)
    a, g = o.chunk(2, dim=-1)
    ref = a * F.gelu(g)
    got = ops.linear(x.to(_dev()).to(dtype), w.to(_dev()), b.to(_dev()), act="geglu")
    check(got, ref, dtype, "geglu")


@pytest.mark.parametrize("M,N,act,bias", [(300, 960, None, False), (1024, 320, None, False), (4096, 2560, "geglu", True), (128, 336, None, True),
                                          (77, 400, None, True), (2, 640, "geglu", True), (32768, 960, None, False), (300, 512, "geglu", True),
                                          (1000, 2560, "geglu", False)])
def test_ln_linear(M, N, act, bias):
    """crg_ln_gemm (LayerNorm fused into the consuming GEMM, K = 320; lngemm.hip) against LayerNorm -> bf16 rounding -> Linear:
    row tails (M % 128 != 0), 160- and 128-wide tiles, the anti-phase GEGLU kernel whose weight ring overlays the resident rows
    (N % 256 == 0), the paired and the plain column mapping, bias, GEGLU, and bitwise
    agreement of the normalised operand with the stand-alone crg_layernorm (same two-pass arithmetic)."""
    from cremage_amd import ops
    K = 320
    x = rnd(M, K, seed=140, scale=2.0) + 0.7
    g, be = 1 + 0.2 * rnd(K, seed=141), 0.3 * rnd(K, seed=142)
    w, b = rnd(N, K, seed=143, scale=K ** -0.5), (rnd(N, seed=144, scale=0.2) if bias else None)
    xq = q(x, BF)
    ln = q(F.layer_norm(xq, (K,), g, be, 1e-5), BF)                 # the MFMA operand is LN(x) rounded to bf16 once
    o = F.linear(ln, q(w, BF), b)
    if act == "geglu":
        a_, g_ = o.chunk(2, dim=-1)
        ref = a_ * F.gelu(g_)
    else:
        ref = o
    dx, dw = x.to(_dev()).to(BF), w.to(_dev()).to(BF)
    assert ops.ln_linear_ok(dx, dw)
    got = ops.ln_linear(dx, g.to(_dev()), be.to(_dev()), 1e-5, dw, b.to(_dev()) if bias else None, act=act)
    check(got, ref, BF, f"ln_linear {M}x{N} {act}")
    two = ops.linear(ops.layer_norm(dx, g.to(_dev()), be.to(_dev()), 1e-5), dw, b.to(_dev()) if bias else None, act=act)
    d = (got.float() - two.float()).abs().max().item()
    # same LN arithmetic up to the order of the fp32 row sums: a few elements of LN(x) may round to the neighbouring bf16
    assert d <= 2 ** -6 * HS * max(1.0, two.float().abs().max().item()), d


@pytest.mark.parametrize("M,N,bias,res", [(4096, 320, True, True), (5000, 320, True, False), (1024, 640, False, True)])
def test_row_resident_gemm_without_layernorm(M, N, bias, res):
    """crg_ln_gemm with gamma = beta = NULL (no LayerNorm) + residual: the row-resident kernel as a plain K = 320 GEMM
    (ops.ln_linear(x, None, None, ...); not routed by default - measured equal to crg_gemm on these shapes)."""
    from cremage_amd import ops
    K = 320
    x, w = rnd(M, K, seed=155), rnd(N, K, seed=156, scale=K ** -0.5)
    b = rnd(N, seed=157, scale=0.2) if bias else None
    r = rnd(M, N, seed=158) if res else None
    ref = F.linear(q(x, BF), q(w, BF), b) + (q(r, BF) if res else 0.0)
    got = ops.ln_linear(x.to(_dev()).to(BF), None, None, 0.0, w.to(_dev()).to(BF), b.to(_dev()) if bias else None,
                        residual=r.to(_dev()).to(BF) if res else None)
    check(got, ref, BF, f"row-resident gemm {M}x{N}")


@pytest.mark.parametrize("B,T", [(2, 256), (3, 100), (8, 4096)])
def test_ln_linear_transposed_v(B, T):
    """crg_ln_gemm with a transposed column range: LayerNorm + Q | K | V in one launch, Q | K row-major and V as V^T [B, C, ld]
    (what crg_attention takes) - against the two-launch form (fused Q | K GEMM + linear_transposed) on the same LN output."""
    from cremage_amd import ops
    K = C = 320
    x = rnd(B, T, K, seed=150, scale=1.5) - 0.2
    g, be = 1 + 0.2 * rnd(K, seed=151), 0.3 * rnd(K, seed=152)
    w = rnd(3 * C, K, seed=153, scale=K ** -0.5)
    dx, dw = x.to(_dev()).to(BF), w.to(_dev()).to(BF)
    qk, vt = ops.ln_linear(dx, g.to(_dev()), be.to(_dev()), 1e-5, dw, transposed_from=2 * C)
    ld = (T + 7) // 8 * 8
    assert qk.shape == (B, T, 2 * C) and vt.shape == (B, C, ld)
    ln = q(F.layer_norm(q(x, BF), (K,), g, be, 1e-5), BF)
    ref = F.linear(ln, q(w, BF))
    check(qk, ref[..., :2 * C], BF, "ln_linear qk")
    check(vt[:, :, :T].transpose(1, 2), ref[..., 2 * C:], BF, "ln_linear v^T")
    assert (vt[:, :, T:] == 0).all()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("T", [77, 154, 64, 1])
def test_linear_transposed(dtype, T):
    from cremage_amd import ops
    x, w, b = rnd(2, T, 96, seed=10), rnd(128, 96, seed=11, scale=0.1), rnd(128, seed=12)
    ref = (F.linear(q(x, dtype), q(w, BF) if dtype == BF else w, b)).transpose(1, 2)
    got = ops.linear_transposed(x.to(_dev()).to(dtype), w.to(_dev()), b.to(_dev()))
    assert got.shape[-1] == (T + 7) // 8 * 8
    check(got[:, :, :T], ref, dtype, "linear_transposed")
    assert (got[:, :, T:] == 0).all()


# ------------------------------------------------------------------------------------------ conv
def conv_ref(x, w, b, dtype, stride=1, pad=(1, 1, 1, 1), up=False, x2=None, cvec=None, res=None):
    xx = q(x, dtype)
    if x2 is not None:
        xx = torch.cat([xx, q(x2, dtype)], dim=1)
    if up:
        xx = F.interpolate(xx, scale_factor=2, mode="nearest")
    pt, pl, pb, pr = pad
    xx = F.pad(xx, (pl, pr, pt, pb))
    y = F.conv2d(xx, q(w, BF) if dtype == BF else w, b, stride=stride)
    if cvec is not None:
        y = y + cvec[:, :, None, None]
    if res is not None:
        y = y + q(res, dtype)
    return y


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("case", ["s1", "s2", "asym", "up", "cat", "cat1x1", "fused", "odd"])
def test_conv2d(dtype, case):
    from cremage_amd import ops
    N, C, Co, H, W = 2, 64, 96, 10, 12
    kw = {}
    rk = {}
    ks = 3
    x2 = None
    if case == "s2":
        kw["stride"] = rk["stride"] = 2
    if case == "asym":
        kw["stride"] = rk["stride"] = 2
        kw["padding"] = rk["pad"] = (0, 0, 1, 1)
    if case == "up":
        kw["upsample2x"] = rk["up"] = True
    if case in ("cat", "cat1x1"):
        x2 = rnd(N, 32, H, W, seed=21)
        if case == "cat1x1":
            ks = 1
            kw["padding"], rk["pad"] = 0, (0, 0, 0, 0)
    if case == "odd":
        N, C, Co, H, W = 1, 40, 72, 7, 5
    Cin = C + (x2.shape[1] if x2 is not None else 0)
    x, w, b = rnd(N, C, H, W, seed=20), rnd(Co, Cin, ks, ks, seed=22, scale=(Cin * ks * ks) ** -0.5), rnd(Co, seed=23)
    cvec = res = None
    if case == "fused":
        cvec = rnd(N, Co, seed=24)
    ref = conv_ref(x, w, b, dtype, x2=x2, cvec=cvec, **rk)
    if case == "fused":
        res = rnd(*ref.shape, seed=25)
        ref = ref + q(res, dtype)
    got = ops.conv2d(nhwc(x, dtype), w.to(_dev()), b.to(_dev()), x2=nhwc(x2, dtype) if x2 is not None else None,
                     cvec=cvec.to(_dev()) if cvec is not None else None, residual=nhwc(res, dtype) if res is not None else None, **kw)
    check(got, ref, dtype, "conv " + case)


_TILE_CONFIG_ROUTES = {
    (2, 64, 320, 96): dict(kernel="glds", config=4, splits=1),                                   # 288 tiles of 128 rows -> D
    (4, 64, 320, 128): dict(kernel="conv_pp", config=1, rowhalo=2, splits=1),                    # 1024 tiles -> A's place: 512 tiles of 256 pixels on conv_pp
    (1, 64, 640, 40): dict(kernel="glds", config=3, splits=1),                                   # 26 tiles of 128 rows -> C
    (4, 128, 320, 96): dict(kernel="rowhalo", config=1, rowhalo=1, halo_lin=1, splits=1, tail_splits=4, reduce="plain")}  # 576 tiles -> tail split


@pytest.mark.parametrize("N,C,Co,hw", list(_TILE_CONFIG_ROUTES))
def test_conv2d_tile_configs(N, C, Co, hw):
    """bf16 3x3 convs sized to land on configurations D (288 tiles of 128 rows) and C (26 tiles of 128 rows) of the generic implicit GEMM,
    and on the two kernels that stand in configuration A's place for 3x3 convs: the 256-pixel-tile kernel (1024 tiles of 128 rows) and the
    row-halo kernel with a K-split tail (576 tiles)."""
    from cremage_amd import ops
    x, w, b = rnd(N, C, hw, hw, seed=30), rnd(Co, C, 3, 3, seed=31, scale=(C * 9) ** -0.5), rnd(Co, seed=32)
    res = rnd(N, Co, hw, hw, seed=33)
    ref = conv_ref(x, w, b, BF) + q(res, BF)
    got = ops.conv2d(nhwc(x, BF), w.to(_dev()), b.to(_dev()), residual=nhwc(res, BF))
    assert_route(f"conv cfg {N}x{C}x{hw}x{hw}->{Co}", **_TILE_CONFIG_ROUTES[(N, C, Co, hw)])
    check(got, ref, BF, f"conv cfg {N}x{C}x{hw}x{hw}->{Co}")


@pytest.mark.parametrize("C,Co,ks", [(64, 96, 3), (32, 64, 3), (128, 160, 3), (128, 3, 3), (64, 128, 1), (40, 64, 1)])
def test_split_planes_path(C, Co, ks):
    """fp32-class operands as pre-split bf16 planes (crg_split_bf16 / crg_groupnorm_split -> crg_conv_args.x_lo): the planes
    reproduce the fp32 tensor to 2^-16, and the 4-plane LDS-DMA conv equals the register-staged fp32-class conv and an fp64
    reference (chunk-major and tap-major weight layouts, 1x1 and 3x3, thin outputs)."""
    from cremage_amd import ops
    x = rnd(2, C, 24, 20, seed=70, scale=3.0) + 1.0
    xd = nhwc(x, torch.float32)
    hi, lo = ops.split_bf16(xd)
    assert hi.dtype == lo.dtype == BF and hi.shape == xd.shape
    rec = hi.float() + lo.float()
    assert ((rec - xd).abs() / xd.abs().clamp_min(1e-3)).max().item() < 2.0 ** -15
    groups = 32 if C % 32 == 0 else 8
    g, b = 1 + 0.1 * rnd(C, seed=71), 0.1 * rnd(C, seed=72)
    ref = ops.group_norm(xd, g.to(_dev()), b.to(_dev()), groups, 1e-6, silu=True)
    gh, gl = ops.group_norm(xd, g.to(_dev()), b.to(_dev()), groups, 1e-6, silu=True, split=True)
    assert (gh.float() + gl.float() - ref).abs().max().item() < 1e-4
    w, bias = rnd(Co, C, ks, ks, seed=73, scale=(C * ks * ks) ** -0.5), rnd(Co, seed=74)
    res = nhwc(rnd(2, Co, 24, 20, seed=75), torch.float32)
    variants = (dict(), dict(residual=res), dict(stride=2, padding=(0, 0, 1, 1)), dict(upsample2x=True)) if ks == 3 else \
        (dict(padding=0), dict(padding=0, residual=res))
    for kw in variants:
        a = ops.conv2d(xd, w.to(_dev()), bias.to(_dev()), **kw)
        bb = ops.conv2d(hi, w.to(_dev()), bias.to(_dev()), x_lo=lo, **kw)
        assert bb.dtype == torch.float32 and bb.shape == a.shape
        assert (a - bb).abs().max().item() < 2e-5 * max(1.0, a.abs().max().item()), kw
        ref64 = F.conv2d(F.interpolate(x.double(), scale_factor=2, mode="nearest") if kw.get("upsample2x") else
                         (F.pad(x.double(), (0, 1, 0, 1)) if kw.get("stride") == 2 else x.double()), w.double(), bias.double(),
                         stride=kw.get("stride", 1), padding=0 if (ks == 1 or kw.get("stride") == 2) else 1)
        if "residual" in kw:
            ref64 = ref64 + res.double().cpu()
        fig(f"planes conv vs fp64 {sorted(kw)}", (bb.double().cpu() - ref64).abs().max().item(), 3e-5 * max(1.0, ref64.abs().max().item()))
        assert (bb.double().cpu() - ref64).abs().max().item() < 3e-5 * max(1.0, ref64.abs().max().item()), ("vs fp64", kw)
    with pytest.raises(Exception):
        ops.conv2d(hi, w.to(_dev()), bias.to(_dev()), x_lo=lo.float())


_GENERIC_C = dict(kernel="glds", config=3, splits=1, rowhalo=0)  # fewer than 192 tiles and a K too short to cut: the generic implicit GEMM


def _halo(splits, lin=0, **kw):
    return dict(dict(kernel="rowhalo", config=1, rowhalo=1, halo_lin=lin, splits=splits, reduce="plain" if splits > 1 else "none"), **kw)


_ROWHALO_ROUTES = {
    # The row-halo kernel exists in configuration A only, which a 3x3 conv reaches with at least 384 tiles of 128 rows or with a K worth
    # cutting (>= 24 k-tiles: Cin >= 192).  The small 64-channel shapes below were written for it but run on configuration C of the
    # generic implicit GEMM; they stay as they are (same geometry on the other kernel) and each has a 192-channel twin that does reach
    # the row-halo kernel.
    (2, 64, 0, 16, 16, 64): _GENERIC_C,       # one chunk
    (2, 192, 0, 16, 16, 64): _halo(3),        # ... row-halo: tiles of 8 image rows
    (1, 128, 64, 24, 32, 160): _halo(3),      # virtual concat, H != W, 160-wide tiles
    (3, 64, 0, 5, 16, 96): _GENERIC_C,        # M = 240: tile tail
    (3, 192, 0, 5, 16, 96): _halo(3),         # ... row-halo: tile tail, tiles straddling images
    (2, 72, 56, 16, 32, 64): _GENERIC_C,      # concat boundary inside a 64-channel chunk
    (2, 136, 56, 16, 32, 64): _halo(3),       # ... row-halo: concat boundary inside the third chunk
    (1, 1280, 0, 16, 16, 128): _halo(16),     # long K: split-K slices in (chunk, kernel row) groups
    (1, 64, 0, 4, 128, 64): _GENERIC_C,       # W = 128
    (1, 192, 0, 4, 128, 64): _halo(3),        # ... row-halo: one image row per tile
    (2, 320, 0, 64, 64, 320): _GENERIC_C,     # SD1.5 64x64 level at batch 2: 128 tiles, 45 k-tiles -> C, unsplit
    (8, 640, 0, 32, 32, 640): dict(kernel="conv_pp", config=1, rowhalo=2, splits=2, reduce="plain"),  # production shape: 128 tiles of 256 pixels x two K slices
    (2, 64, 0, 9, 7, 64): _GENERIC_C,         # width 7, M = 126 (one partial tile)
    (2, 192, 0, 9, 7, 64): _halo(3, 1),       # ... row-halo, linear-pixel row buffer
    (2, 128, 64, 24, 40, 96): _halo(3, 1),    # linear: ragged latent, concat
    (1, 320, 0, 96, 96, 320): _GENERIC_C,     # 768x768 image level at batch 1: 144 tiles -> C (test_conv_256_pixel_tile_shapes has the linear buffer on 256-row tiles)
    (3, 64, 0, 8, 8, 64): _GENERIC_C,         # 8x8 level
    (3, 192, 0, 8, 8, 64): _halo(3, 1),       # ... row-halo, linear: tiles straddling images
    (1, 64, 0, 2, 200, 64): _GENERIC_C,       # W = 200
    (1, 192, 0, 2, 200, 64): _halo(3, 1),     # ... row-halo, linear: rows longer than a tile
    (4, 128, 0, 96, 96, 320): _halo(1, 1, tail_splits=4, reduce="plain"),  # 576 tiles = 512 + 64: tail split (second launch cut along K in row groups) on the linear buffer
    (1, 64, 0, 777, 16, 640): _halo(1, tail_splits=0),  # 98 x 4 = 392 tiles, 9 k-tiles: unsplit grid with a ragged last tile (M = 97 * 128 + 16)
}


@pytest.mark.parametrize("N,C1,C2,H,W,Co", list(_ROWHALO_ROUTES))
def test_conv_rowhalo_shapes(N, C1, C2, H, W, Co):
    """3x3 / stride 1 / pad 1 convs on conv3_rowhalo_kernel (one halo'd row buffer per kernel row instead of one activation tile per
    tap) - and, for the shapes too small to reach it, on the generic implicit GEMM: image borders, tile tails, concat inputs, split-K
    and every fused epilogue term.  Each case asserts the kernel it ran."""
    from cremage_amd import ops
    C = C1 + C2
    x = rnd(N, C1, H, W, seed=80)
    x2 = rnd(N, C2, H, W, seed=81) if C2 else None
    w, b = rnd(Co, C, 3, 3, seed=82, scale=(9 * C) ** -0.5), rnd(Co, seed=83)
    res, cvec = rnd(N, Co, H, W, seed=84), rnd(N, Co, seed=85)
    for kw in (dict(), dict(res=res), dict(cvec=cvec, res=res)):
        ref = conv_ref(x, w, b, BF, x2=x2, **kw)
        got = ops.conv2d(nhwc(x, BF), w.to(_dev()), b.to(_dev()), x2=nhwc(x2, BF) if C2 else None,
                         cvec=kw["cvec"].to(_dev()) if "cvec" in kw else None, residual=nhwc(kw["res"], BF) if "res" in kw else None)
        assert_route(f"rowhalo conv {N}x{C1}+{C2}x{H}x{W}->{Co} {sorted(kw)}", **_ROWHALO_ROUTES[(N, C1, C2, H, W, Co)])
        check(got, ref, BF, f"rowhalo conv {N}x{C1}+{C2}x{H}x{W}->{Co} {sorted(kw)}")


@pytest.mark.parametrize("N,C1,C2,H,W,Co,up", [
    (8, 320, 0, 64, 64, 320, False),    # 256 tiles of 256 x 160: one round, no split-K (SD1.5 64x64 level)
    (8, 320, 320, 64, 64, 320, False),  # ... with the skip concat (second pointer switches at a chunk boundary)
    (8, 640, 0, 32, 32, 640, False),    # 128 tiles x 2 K slices
    (8, 1280, 0, 16, 16, 1280, False),  # 64 tiles x 4 K slices, 16 whole image rows per tile
    (8, 1280, 0, 8, 8, 1280, False),    # linear-pixel row buffer (8x8 level), 16 K slices
    (8, 640, 0, 32, 32, 640, True),     # nearest-2x upsample folded into the gather, 64x64 output
    (8, 192, 64, 64, 64, 128, False),   # 128 outputs = one n-tile: 128 blocks of 256 pixels fill half a round, below the 85 % rule -> 64-row tiles (D) of the generic kernel
    (14, 64, 64, 64, 64, 128, False),   # ... 224 blocks do: conv_pp with 128-wide tiles (WNT = 4), concat
    (2, 128, 0, 128, 128, 320, False),  # W = 128 divides the tile: two image rows per tile
    (1, 128, 0, 64, 512, 320, False),   # W = 512 > tile: one 256-pixel row SEGMENT per tile
])
def test_conv_256_pixel_tile_shapes(N, C1, C2, H, W, Co, up):
    """3x3 convs whose grid fills rounds of 256-pixel tiles run on conv3_pp_kernel (conv_pp.hip: 4-slot weight ring, counted vmcnt,
    the two waves of a SIMD half a k-tile apart): every buffer geometry, split-K, concat, upsample and epilogue term."""
    from cremage_amd import ops
    splits = {(8, 640, 32, False): 2, (8, 1280, 16, False): 4, (8, 1280, 8, False): 16}.get((N, C1, H, up), 1)
    route = dict(kernel="conv_pp", config=1, rowhalo=2, wnt=4 if Co == 128 else 5, splits=splits, halo_lin=1 if W == 8 else 0, reduce="plain" if splits > 1 else "none")
    if (N, Co) == (8, 128):
        route = dict(kernel="glds", config=4, wnt=4, splits=1, rowhalo=0)
    C = C1 + C2
    x = rnd(N, C1, H, W, seed=180)
    x2 = rnd(N, C2, H, W, seed=181) if C2 else None
    w, b = rnd(Co, C, 3, 3, seed=182, scale=(9 * C) ** -0.5), rnd(Co, seed=183)
    Ho, Wo = (2 * H, 2 * W) if up else (H, W)
    res, cvec = rnd(N, Co, Ho, Wo, seed=184), rnd(N, Co, seed=185)
    for kw in (dict(), dict(cvec=cvec, res=res)):
        ref = conv_ref(x, w, b, BF, x2=x2, up=up, **kw)
        got = ops.conv2d(nhwc(x, BF), w.to(_dev()), b.to(_dev()), x2=nhwc(x2, BF) if C2 else None, upsample2x=up,
                         cvec=kw["cvec"].to(_dev()) if "cvec" in kw else None, residual=nhwc(kw["res"], BF) if "res" in kw else None)
        assert_route(f"ring conv {N}x{C1}+{C2}x{H}x{W}->{Co} up={up} {sorted(kw)}", **route)
        check(got, ref, BF, f"ring conv {N}x{C1}+{C2}x{H}x{W}->{Co} up={up} {sorted(kw)}")


@pytest.mark.parametrize("N,C1,C2,H,W,Co,res", [
    (8, 1280, 0, 16, 16, 1280, False),   # 4 K slices: the reduce launch normalises (5 vectors per thread)
    (8, 1280, 0, 8, 8, 1280, True),      # 16 K slices, linear row buffer, residual
    (8, 1280, 1280, 8, 8, 1280, False),  # skip concat in front
    (2, 640, 0, 16, 16, 1280, False),    # fewer samples: other split count
    (8, 640, 0, 32, 32, 640, False),     # 1024 pixels x 20-channel groups: gs % 8 != 0 -> raises (checked below)
    (2, 128, 0, 16, 16, 256, False),     # not split along K: conv, then the GroupNorm as its own launch
])
def test_conv_gn_fused(N, C1, C2, H, W, Co, res):
    """crg_conv_args.gn_y: conv (+bias +cvec +residual) and the GroupNorm + SiLU behind it in one call - bitwise the two separate
    calls (the fused split-K reduce repeats their arithmetic), and the reference's values."""
    from cremage_amd import ops
    C = C1 + C2
    x = rnd(N, C1, H, W, seed=280)
    x2 = rnd(N, C2, H, W, seed=281) if C2 else None
    w, b = rnd(Co, C, 3, 3, seed=282, scale=(9 * C) ** -0.5), rnd(Co, seed=283)
    cvec, r = rnd(N, Co, seed=284), rnd(N, Co, H, W, seed=285)
    g, be = (1 + 0.1 * rnd(Co, seed=286)).to(_dev()), (0.1 * rnd(Co, seed=287)).to(_dev())
    kw = dict(x2=nhwc(x2, BF) if C2 else None, cvec=cvec.to(_dev()), residual=nhwc(r, BF) if res else None)
    xd, wd, bd = nhwc(x, BF), w.to(_dev()), b.to(_dev())
    if (Co // 32) % 8:
        with pytest.raises(Exception):
            ops.conv2d(xd, wd, bd, gn=(g, be, 32, 1e-5, True), **kw)
        return
    y, yn = ops.conv2d(xd, wd, bd, gn=(g, be, 32, 1e-5, True), **kw)
    y2 = ops.conv2d(xd, wd, bd, **kw)
    yn2 = ops.group_norm(y2, g, be, 32, 1e-5, silu=True)
    assert torch.equal(y, y2), "raw output differs from the plain conv"
    assert torch.equal(yn, yn2), "fused GroupNorm differs from conv -> group_norm"
    ref = conv_ref(x, w, b, BF, x2=x2, cvec=cvec, **(dict(res=r) if res else {}))
    check(y, ref, BF, "conv_gn raw")
    refn = F.silu(F.group_norm(y2.float().cpu(), 32, g.cpu(), be.cpu(), 1e-5))
    check(yn, refn, BF, "conv_gn normalised")


def _mx_decode(x8, c, hi_log2, lo_log2):
    """(hi8, lo8) planes of an MX pair plane [..., 2 C] uint8 as fp32 tensors [..., C] with the scales undone"""
    v = x8.view(torch.float8_e4m3fn).float().reshape(x8.shape[:-1] + (c // 64, 2, 64))
    return (v[..., 0, :] * 2.0 ** -hi_log2).reshape(x8.shape[:-1] + (c,)), (v[..., 1, :] * 2.0 ** -lo_log2).reshape(x8.shape[:-1] + (c,))


def test_mx_planes_of_split_and_groupnorm():
    """crg_split_mx / crg_groupnorm_mx: the fp16 plane is half(x); the pair plane holds OCP e4m3 of half(x) * 2^4 and of (x - half(x)) * 2^15
    (saturating) per 64-channel chunk - decoded here with torch's float8_e4m3fn, so an encoding mismatch (fnuz) would show as a factor 2."""
    from cremage_amd import ops
    dev = _dev()
    x = rnd(2, 128, 16, 32, seed=601) * 3.0
    x[0, 5, 3, 7] = 100.0  # beyond the hi8 range: saturates at 28, must not wrap
    xd = nhwc(x, torch.float32)
    x16, x8 = ops.split_mx(xd)
    ref16 = x.to(torch.float16)
    assert torch.equal(x16.cpu().contiguous(), ref16)
    hi, lo = _mx_decode(x8.cpu(), 128, *ops.MX_X_LOG2)
    xl = x.permute(0, 2, 3, 1)
    h16 = ref16.float().permute(0, 2, 3, 1)
    sat = h16.clamp(-28.0, 28.0)
    assert ((hi - sat).abs() <= sat.abs() * 2.0 ** -4 + 2.0 ** -13).all()           # 3 mantissa bits, subnormals below 2^-6 / 16
    assert ((lo - (xl - h16)).abs() <= (xl - h16).abs() * 2.0 ** -4 + 2.0 ** -24).all()
    assert abs(hi[0, 3, 7, 5].item() - 28.0) < 1e-6
    g, be = 1.0 + 0.2 * rnd(128, seed=602), 0.1 * rnd(128, seed=603)
    y16, y8 = ops.group_norm(xd, g.to(dev), be.to(dev), 32, 1e-6, silu=True, split="mx")
    ref = F.silu(F.group_norm(x, 32, g, be, 1e-6))
    assert ((y16.float().cpu() - ref).abs() <= ref.abs() * 2.0 ** -10 + 1e-6).all()
    hi, lo = _mx_decode(y8.cpu(), 128, *ops.MX_X_LOG2)
    rec = y16.float().cpu().permute(0, 2, 3, 1) + lo                                    # fp16 plane + lo8 remainder ~ the fp32 value
    assert ((rec - ref.permute(0, 2, 3, 1)).abs() <= ref.permute(0, 2, 3, 1).abs() * 2.0 ** -14 + 1e-6).all()


@pytest.mark.parametrize("N,C,H,W,Co,res", [(2, 128, 32, 32, 128, True),     # rows mode (four image rows per tile), one n-tile
                                            (1, 256, 16, 64, 256, False),    # two image rows per tile
                                            (1, 128, 8, 256, 128, True),     # row segments
                                            (2, 64, 6, 24, 64, False),       # linear buffer (width 24), three k-tiles per slice group: odd k-tile counts
                                            (2, 512, 8, 8, 512, True),       # split-K: slices of an odd number of k-tiles end on a half pair
                                            (1, 128, 64, 64, 512, False),    # four n-tiles
                                            (1, 192, 16, 16, 320, False)])   # 160-wide tiles (the spilling instantiation still has to be right)
def test_conv_mx(N, C, H, W, Co, res):
    """CRG_PREC_F16MX: the fp32-class 3x3 conv as one fp16 pass + two cross terms on the block-scaled MX matrix instruction, against the fp32
    torch conv: per-op error ~1e-5 (bf16 x 3: ~1e-5; one fp16 pass alone: 2e-4), every buffer geometry of the row-halo kernel, split-K with
    odd k-tile counts, GroupNorm statistics out of the epilogue."""
    from cremage_amd import ops
    dev = _dev()
    x = rnd(N, C, H, W, seed=610)
    w, b = rnd(Co, C, 3, 3, seed=611, scale=(9 * C) ** -0.5), rnd(Co, seed=612)
    r = rnd(N, Co, H, W, seed=613) if res else None
    ref = F.conv2d(x, w, b, padding=1) + (r if res else 0)
    x16, x8 = ops.split_mx(nhwc(x, torch.float32))
    y = ops.conv2d(x16, w.to(dev), b.to(dev), x_mx=x8, residual=nhwc(r, torch.float32) if res else None, gn_stats=True)
    assert y.dtype == torch.float32
    rel = ((y.cpu() - ref).norm() / ref.norm()).item()
    one_pass = ((F.conv2d(x.half().float(), w.half().float(), b, padding=1) + (r if res else 0) - ref).norm() / ref.norm()).item()
    assert rel < 4e-5 and rel < 0.3 * one_pass, (rel, one_pass)
    st = getattr(y, "_crg_gn", None)
    if H * W % 32 == 0 and H * W >= 512:
        assert st is not None
        s0 = st[0][0].double().cpu().reshape(N, -1, Co).sum(1)
        assert (s0 - y.double().cpu().sum(dim=(2, 3))).abs().max().item() < 1e-3 * y.abs().sum(dim=(2, 3)).max().item()


@pytest.mark.parametrize("N,C,H,W,Co", [(2, 64, 8, 8, 64), (1, 128, 16, 32, 160), (1, 64, 3, 64, 64), (1, 64, 2, 128, 64), (2, 64, 5, 12, 96)])
def test_conv_rowhalo_upsample(N, C, H, W, Co):
    """nearest-2x upsample folded into the row-halo conv's gather (output-grid geometry, sources at (h >> 1, w >> 1)):
    whole-row, row-segment and linear buffers."""
    from cremage_amd import ops
    x, w, b = rnd(N, C, H, W, seed=95), rnd(Co, C, 3, 3, seed=96, scale=(9 * C) ** -0.5), rnd(Co, seed=97)
    ref = conv_ref(x, w, b, BF, up=True)
    got = ops.conv2d(nhwc(x, BF), w.to(_dev()), b.to(_dev()), upsample2x=True)
    check(got, ref, BF, f"rowhalo upsample conv {N}x{C}x{H}x{W}->{Co}")


@pytest.mark.parametrize("N,C,H,W,Co", [(1, 64, 16, 16, 64), (2, 128, 8, 32, 128), (1, 128, 6, 256, 96), (1, 256, 16, 64, 160),
                                          (1, 64, 3, 128, 64), (3, 64, 5, 16, 32), (2, 64, 24, 20, 96), (1, 128, 5, 96, 128)])
def test_conv_rowhalo_planes(N, C, H, W, Co):
    """The fp32-class (split-plane) form of the row-halo conv, incl. 128-pixel row segments of wider images, against fp64."""
    from cremage_amd import ops
    x = rnd(N, C, H, W, seed=90, scale=2.0) + 0.5
    w, b = rnd(Co, C, 3, 3, seed=91, scale=(9 * C) ** -0.5), rnd(Co, seed=92)
    res = rnd(N, Co, H, W, seed=93)
    hi, lo = ops.split_bf16(nhwc(x, torch.float32))
    for with_res in (False, True):
        ref = F.conv2d(x.double(), w.double(), b.double(), padding=1) + (res.double() if with_res else 0.0)
        got = ops.conv2d(hi, w.to(_dev()), b.to(_dev()), x_lo=lo, residual=nhwc(res, torch.float32) if with_res else None)
        assert got.dtype == torch.float32
        err = fig("row-halo planes conv vs fp64", (got.double().cpu() - ref).abs().max().item(), 3e-5 * max(1.0, ref.abs().max().item()))
        assert err < 3e-5 * max(1.0, ref.abs().max().item()), (N, C, H, W, Co, with_res, err)


@pytest.mark.parametrize("N,C,H,W,Co,with_res", [(2, 128, 32, 32, 128, False), (1, 64, 16, 128, 256, True), (2, 256, 64, 64, 128, True)])
def test_conv_planes_gn_stats(N, C, H, W, Co, with_res):
    """fp32-class conv on split planes with the GroupNorm statistics side channel (fp32 epilogue), then crg_groupnorm_pre_split: the
    statistics planes equal the per-32-row-block sums of the conv's own output, and the normalised planes equal GroupNorm + swish of it
    (fp64 reference) as closely as the path that reads the tensor for its statistics."""
    from cremage_amd import ops
    x = rnd(N, C, H, W, seed=190, scale=2.0) + 0.5
    w, b = rnd(Co, C, 3, 3, seed=191, scale=(9 * C) ** -0.5), rnd(Co, seed=192) + 1.5  # a mean well away from zero
    res = rnd(N, Co, H, W, seed=193)
    g, be = (1 + 0.1 * rnd(Co, seed=194)).to(_dev()), (0.1 * rnd(Co, seed=195)).to(_dev())
    hi, lo = ops.split_bf16(nhwc(x, torch.float32))
    y = ops.conv2d(hi, w.to(_dev()), b.to(_dev()), x_lo=lo, residual=nhwc(res, torch.float32) if with_res else None, gn_stats=True)
    assert_route(f"planes conv + statistics {N}x{C}x{H}x{W}->{Co}", kernel="planes", rowhalo=1, splits=1, reduce="none", mx=0, gn_stats_rows=32)
    st = getattr(y, "_crg_gn", None)
    assert st is not None, "the planes conv did not attach its statistics"
    rows = y.permute(0, 2, 3, 1).reshape(-1, Co).double()                      # [M][Co] in the kernel's row order
    blk = rows.reshape(-1, 32, Co)
    assert (st[0][0].double() - blk.sum(1)).abs().max().item() < 2e-4 * max(1.0, blk.sum(1).abs().max().item())
    assert (st[0][1].double() - (blk * blk).sum(1)).abs().max().item() < 2e-4 * max(1.0, (blk * blk).sum(1).abs().max().item())
    nh, nl = ops.group_norm(y, g, be, 32, 1e-6, silu=True, split=True)          # consumes the statistics
    y2 = y.clone()                                                             # same values, no side channel: the statistics kernel
    rh, rl = ops.group_norm(y2, g, be, 32, 1e-6, silu=True, split=True)
    ref = F.silu(F.group_norm(y.double().cpu(), 32, g.double().cpu(), be.double().cpu(), 1e-6))
    e_pre = ((nh.float() + nl.float()).double().cpu() - ref).abs().max().item()
    e_ref = ((rh.float() + rl.float()).double().cpu() - ref).abs().max().item()
    fig("GroupNorm planes from conv statistics vs fp64", e_pre, 1e-4)
    assert e_pre < 1e-4 and e_pre < 1.5 * e_ref + 1e-6, (e_pre, e_ref)  # the planes' own resolution (hi + lo: 2^-17 relative) bounds both
    st[0].zero_()                                                              # ... and the side channel really is what was consumed
    zh, _ = ops.group_norm(y, g, be, 32, 1e-6, silu=True, split=True)
    assert not torch.equal(zh, nh)


@pytest.mark.parametrize("dtype", DTYPES)
def test_conv_unet_shapes(dtype):
    """production channel counts at small spatial size (tile tails in both M and N)"""
    from cremage_amd import ops
    for (ci, co, hw) in [(320, 320, 8), (640, 1280, 4), (960, 640, 6)]:
        x, w, b = rnd(2, ci, hw, hw, seed=30), rnd(co, ci, 3, 3, seed=31, scale=(9 * ci) ** -0.5), rnd(co, seed=32)
        check(ops.conv2d(nhwc(x, dtype), w.to(_dev()), b.to(_dev())), conv_ref(x, w, b, dtype), dtype, f"conv {ci}->{co}")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("ci,co,ks,h,w", [(4, 320, 3, 6, 12), (3, 128, 3, 5, 8), (4, 64, 1, 3, 4), (4, 320, 3, 64, 64)])
def test_conv_small_four_pixels_per_thread(dtype, ci, co, ks, h, w):
    """conv_in form with W % 4 == 0: four pixels of a row share every weight read (borders inside a quad, the production 64x64 shape)"""
    from cremage_amd import ops
    x, wt, b = rnd(2, ci, h, w, seed=43), rnd(co, ci, ks, ks, seed=44, scale=(ci * ks * ks) ** -0.5), rnd(co, seed=45)
    ref = F.conv2d(q(x, dtype), wt, b, padding=ks // 2)
    got = ops.conv2d(nhwc(x, dtype), wt.to(_dev()), b.to(_dev()), padding=ks // 2)
    check(got, ref, dtype, f"conv_small quad {ci}->{co} k{ks} {h}x{w}")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("ci,co,ks", [(4, 64, 3), (4, 320, 3), (3, 128, 3), (320, 4, 3), (128, 3, 3), (64, 8, 3), (8, 8, 1), (4, 4, 1)])
def test_conv_small(dtype, ci, co, ks):
    from cremage_amd import ops
    x, w, b = rnd(2, ci, 9, 7, seed=40), rnd(co, ci, ks, ks, seed=41, scale=(ci * ks * ks) ** -0.5), rnd(co, seed=42)
    ref = F.conv2d(q(x, dtype), w, b, padding=ks // 2)
    got = ops.conv2d(nhwc(x, dtype), w.to(_dev()), b.to(_dev()), padding=ks // 2)
    check(got, ref, dtype, f"conv_small {ci}->{co} k{ks}")


# ------------------------------------------------------------------------------------------ norms
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("C,hw,eps", [(64, 8, 1e-5), (320, 12, 1e-5), (128, 33, 1e-6), (1280, 4, 1e-5), (32, 16, 1e-6),
                                          (1280, 16, 1e-5), (2560, 16, 1e-5), (256, 32, 1e-6), (2560, 8, 1e-5)])  # last four: single-launch path
@pytest.mark.parametrize("silu", [False, True])
def test_group_norm(dtype, C, hw, eps, silu):
    from cremage_amd import ops
    x = rnd(2, C, hw, hw, seed=50, scale=2.0) + 3.0  # large mean: exercises the shifted statistics
    g, b = 1 + 0.1 * rnd(C, seed=51), 0.1 * rnd(C, seed=52)
    ref = F.group_norm(q(x, dtype), 32, g, b, eps)
    if silu:
        ref = F.silu(ref)
    got = ops.group_norm(nhwc(x, dtype), g.to(_dev()), b.to(_dev()), 32, eps, silu=silu)
    check(got, ref, dtype, "group_norm")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("tag", ["gn32_e5", "gn32_e5_c320", "gn_e6"])
def test_group_norm_golden(dtype, tag):
    """crg_groupnorm against the fixtures the reference's own GroupNorm32 (util.py:199-216, eps 1e-5) and Normalize
    (attention.py:189-190, eps 1e-6) produced, with and without the fused SiLU (openaimodel.py:205-209)."""
    from cremage_amd import ops
    from cremage_amd.synth import synth_input
    from tests.conftest import load_golden, synth_state_dict
    meta, g = load_golden("op_" + tag)
    C, hw = meta["C"], meta["hw"]
    x = synth_input(tag, (2, C, hw, hw), meta["seed"], 1.5) + 0.3
    sd = synth_state_dict(torch.nn.GroupNorm(32, C), meta["seed"], meta["prefix"])
    w, b = sd["weight"].to(_dev()), sd["bias"].to(_dev())
    for silu, key in ((False, "y"), (True, "y_silu")):
        got = ops.group_norm(nhwc(x, dtype), w, b, 32, meta["eps"], silu=silu)
        ref = g[key]
        err = (got.float().cpu() - ref).abs().max().item()
        # bf16: the input itself is rounded to 8 bits before the statistics (|x| <= ~5 -> 2e-2 of output units after the 1/sigma gain)
        assert err < (2e-5 if dtype == torch.float32 else 6e-2 * HS), (tag, silu, err)
        rel = ((got.float().cpu() - ref).norm() / ref.norm()).item()
        assert rel < (1e-5 if dtype == torch.float32 else 6e-3 * HS), (tag, silu, rel)


@pytest.mark.parametrize("N,C1,C2,hw,silu", [(8, 320, 0, 64, True), (8, 640, 0, 32, True), (8, 320, 0, 64, False), (8, 320, 320, 64, True),
                                               (2, 320, 0, 64, True), (8, 1280, 640, 32, True), (3, 320, 0, 40, True), (8, 640, 320, 64, True)])
def test_group_norm_production_shapes(N, C1, C2, hw, silu):
    """GroupNorm(+SiLU) at the 64x64 / 32x32 levels' production shapes (stats + apply pair): virtual concat, a ragged size,
    repeated calls and bitwise run-to-run determinism (fixed-order reductions, no float atomics)."""
    from cremage_amd import ops
    C = C1 + C2
    x = rnd(N, C1, hw, hw, seed=160, scale=2.0) + 1.5
    x2 = (rnd(N, C2, hw, hw, seed=161, scale=0.5) - 2.0) if C2 else None
    g, b = 1 + 0.1 * rnd(C, seed=162), 0.1 * rnd(C, seed=163)
    xx = q(x, BF) if x2 is None else torch.cat([q(x, BF), q(x2, BF)], dim=1)
    ref = F.group_norm(xx, 32, g, b, 1e-5)
    if silu:
        ref = F.silu(ref)
    dx, dx2 = nhwc(x, BF), (nhwc(x2, BF) if C2 else None)
    outs = [ops.group_norm(dx, g.to(_dev()), b.to(_dev()), 32, 1e-5, silu=silu, x2=dx2) for _ in range(3)]
    check(outs[0], ref, BF, f"gn single launch {N}x{C1}+{C2}x{hw}")
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[1], outs[2])


def _stats_ref(y, hw, rows=32):
    """per `rows`-row block (32, or the producer's tile height) and channel: sum / sum of squares of a channels-last bf16 image, as the
    producers' side channel defines it"""
    n, c, hh, ww = y.shape
    t = y.permute(0, 2, 3, 1).reshape(n * hh * ww // rows, rows, c).float()
    return torch.stack([t.sum(1), (t * t).sum(1)])


_GN_STATS_ROUTES = {
    "conv_unsplit": dict(kernel="conv_pp", rowhalo=2, splits=1, pair=1, reduce="none", gn_stats_rows=256),       # tile partials
    "conv_splitk": dict(kernel="conv_pp", rowhalo=2, splits=8, reduce="stats", gn_stats_rows=32),
    # 576 tiles, but 9 k-tiles are too few for a K-split tail (and the paired epilogue is in use): the row-halo kernel on a grid whose
    # second round is 1/8 full.  The id keeps its old name.
    "conv_pairless_tail": dict(kernel="rowhalo", rowhalo=1, splits=1, tail_splits=0, pair=1, reduce="none", gn_stats_rows=32),
    "conv_tail_split": dict(kernel="rowhalo", rowhalo=1, splits=1, tail_splits=4, pair=1, reduce="stats", gn_stats_rows=32),  # 18 k-tiles: the tail's reduce writes its rows' statistics
    "conv_stride2": dict(kernel="glds", config=3, splits=1, pair=1, reduce="none", gn_stats_rows=32),
    "linear_cfgA": dict(kernel="glds", config=1, splits=1, pair=1, reduce="none", gn_stats_rows=32),
    "linear_cfgC": dict(kernel="glds", config=3, splits=1, pair=1, reduce="none", gn_stats_rows=32),
    "linear_cfgD": dict(kernel="glds", config=4, splits=1, pair=1, reduce="none", gn_stats_rows=32),
}


@pytest.mark.parametrize("case", ["conv_unsplit", "conv_splitk", "conv_pairless_tail", "conv_tail_split", "linear_cfgA", "linear_cfgC", "linear_cfgD", "conv_stride2"])
def test_gn_stats_side_channel(case):
    """The GroupNorm statistics a conv / linear writes next to its output (crg_*_args.gn_stats) equal the sums over its STORED bf16
    output, on every code path that writes them: the paired epilogue (three tile configurations of the GEMM, the row-halo conv, the
    256-pixel ring conv with tile partials), the split-K reduce kernel (whole problem, and the rows of a K-split tail), a stride-2 conv;
    and group_norm() on such a tensor equals group_norm() with its own statistics pass."""
    from cremage_amd import ops
    dev = _dev()
    if case.startswith("conv"):
        N, Cin, Cout, hw, stride = {"conv_unsplit": (8, 64, 320, 64, 1), "conv_splitk": (2, 640, 640, 32, 1), "conv_pairless_tail": (9, 64, 320, 64, 1),
                                    "conv_tail_split": (9, 128, 320, 64, 1), "conv_stride2": (4, 128, 320, 64, 2)}[case]
        x = rnd(N, Cin, hw, hw, seed=200)
        w, b = rnd(Cout, Cin, 3, 3, seed=201, scale=(9 * Cin) ** -0.5), rnd(Cout, seed=202)
        cv = rnd(N, Cout, seed=203).to(dev)
        ho = hw // stride
        r = rnd(N, Cout, ho, ho, seed=204)
        y = ops.conv2d(nhwc(x, BF), w.to(dev), b.to(dev), stride=stride, padding=1, cvec=cv, residual=nhwc(r, BF), gn_stats=True)
        assert_route(case, **_GN_STATS_ROUTES[case])
        ref = F.conv2d(q(x, BF), q(w, BF), b, stride=stride, padding=1) + cv.cpu()[:, :, None, None] + q(r, BF)
        C = Cout
    else:
        M, Nn, K, hw = {"linear_cfgA": (32768, 320, 320, 4096), "linear_cfgC": (2048, 1280, 1280, 1024), "linear_cfgD": (8192, 640, 640, 1024)}[case]
        x, w, b, r = rnd(M, K, seed=210), rnd(Nn, K, seed=211, scale=K ** -0.5), rnd(Nn, seed=212), rnd(M, Nn, seed=213)
        side = int(hw ** 0.5)
        t = ops.linear(x.to(dev).to(BF).view(M // hw, hw, K), w.to(dev), b.to(dev), residual=r.to(dev).to(BF).view(M // hw, hw, Nn), gn_hw=hw)
        assert_route(case, **_GN_STATS_ROUTES[case])
        y = ops.image_of_stats(t, side, side)
        ref = (F.linear(q(x, BF), q(w, BF), b) + q(r, BF)).view(M // hw, side, side, Nn).permute(0, 3, 1, 2)
        C = Nn
    check(y, ref, BF, case)
    g = getattr(y, "_crg_gn", None)
    assert g is not None, "the producer did not hand over statistics"
    rows = g[3] if len(g) > 3 else 32
    want = _stats_ref(y.float().cpu(), g[2], rows)
    assert g[0].shape[1] * 32 == want.shape[1] * rows  # the buffer has the 32-row layout's size; tile partials fill its first M / rows rows
    st = g[0][:, :want.shape[1]].cpu()
    assert st.shape == want.shape
    assert (st[0] - want[0]).abs().max().item() < 1e-3 * max(1.0, want[0].abs().max().item())
    assert (st[1] - want[1]).abs().max().item() < 1e-4 * want[1].abs().max().item()
    gam, bet = (1 + 0.1 * rnd(C, seed=220)).to(dev), (0.1 * rnd(C, seed=221)).to(dev)
    fast = ops.group_norm(y, gam, bet, 32, 1e-5, silu=True)
    again = ops.group_norm(y, gam, bet, 32, 1e-5, silu=True)
    assert torch.equal(fast, again)  # fixed-order folds: bitwise reproducible
    plain = ops.group_norm(y.clone(memory_format=torch.preserve_format), gam, bet, 32, 1e-5, silu=True)  # a clone carries no statistics
    refn = F.silu(F.group_norm(y.float().cpu(), 32, gam.cpu(), bet.cpu(), 1e-5))
    check(fast, refn, BF, case + " gn(pre)")
    assert (fast.float() - plain.float()).abs().max().item() <= 2 ** -6 * HS * refn.abs().max().item()
    # written since: the statistics are stale and must not be used
    y.add_(1.0)
    assert ops._gn_stats_of(y, g[2]) is None
    check(ops.group_norm(y, gam, bet, 32, 1e-5, silu=True), F.silu(F.group_norm(y.float().cpu(), 32, gam.cpu(), bet.cpu(), 1e-5)), BF, case + " stale")


def test_gn_stats_concat_pair():
    """virtual concat of two producers' outputs (the output blocks' GroupNorm over [h, skip], openaimodel.py:808): groups that
    straddle the two tensors take their channels from both side channels (960 = 640 + 320 channels: group size 30)."""
    from cremage_amd import ops
    dev = _dev()
    xa, xb = rnd(2, 64, 32, 32, seed=230), rnd(2, 64, 32, 32, seed=231)
    wa, wb = rnd(640, 64, 3, 3, seed=232, scale=0.05), rnd(320, 64, 3, 3, seed=233, scale=0.05)
    ya = ops.conv2d(nhwc(xa, BF), wa.to(dev), None, padding=1, gn_stats=True)
    yb = ops.conv2d(nhwc(xb, BF), wb.to(dev), None, padding=1, gn_stats=True)
    assert getattr(ya, "_crg_gn", None) is not None and getattr(yb, "_crg_gn", None) is not None
    gam, bet = (1 + 0.1 * rnd(960, seed=234)).to(dev), (0.1 * rnd(960, seed=235)).to(dev)
    got = ops.group_norm(ya, gam, bet, 32, 1e-5, silu=True, x2=yb)
    ref = F.silu(F.group_norm(torch.cat([ya.float().cpu(), yb.float().cpu()], 1), 32, gam.cpu(), bet.cpu(), 1e-5))
    check(got, ref, BF, "gn(pre) concat")


def test_gn_tile_partials():
    """Round 4: the staggered 256-pixel-tile conv folds its waves' sums itself and reports ONE partial per tile and channel
    (crg_conv_args.gn_stats_rows = 256); crg_groupnorm_pre then folds them inside the normalising launch.  The partials equal the sums
    over the stored output; GroupNorm over such a tensor, over a virtual concat of two of them (640 + 320 channels: groups that straddle
    the producers), over a tile-partial tensor next to a 32-row one (the finalise kernel, per-producer granularity) and over a
    batch-doubled copy (ops.dup_batch) equals the reference."""
    from cremage_amd import ops
    dev = _dev()
    if not ops.knobs.GN_TILE:
        pytest.skip("CRG_GN_TILE=0")
    N, hw = 8, 64  # the UNet's own 64x64-level shapes (one 256-pixel tile per CU and more)

    def conv(cin, cout, seed):
        x = rnd(N, cin, hw, hw, seed=seed)
        w, b = rnd(cout, cin, 3, 3, seed=seed + 1, scale=(9 * cin) ** -0.5), rnd(cout, seed=seed + 2)
        r = rnd(N, cout, hw, hw, seed=seed + 3)
        return ops.conv2d(nhwc(x, BF), w.to(dev), b.to(dev), padding=1, residual=nhwc(r, BF), gn_stats=True)

    ya, yb = conv(320, 640, 300), conv(320, 320, 310)
    for y in (ya, yb):
        g = y._crg_gn
        assert len(g) > 3 and g[3] == 256, "the 64x64-level 3x3 conv is expected on the 256-pixel-tile kernel with tile statistics"
        want = _stats_ref(y.float().cpu(), g[2], 256)
        st = g[0][:, :want.shape[1]].cpu()
        assert (st[0] - want[0]).abs().max().item() < 1e-3 * max(1.0, want[0].abs().max().item())
        assert (st[1] - want[1]).abs().max().item() < 1e-4 * want[1].abs().max().item()

    def gn_ref(*ys):
        cat = torch.cat([v.float().cpu() for v in ys], 1)
        c = cat.shape[1]
        gam, bet = 1 + 0.1 * rnd(c, seed=320 + c), 0.1 * rnd(c, seed=321 + c)
        return gam.to(dev), bet.to(dev), F.silu(F.group_norm(cat, 32, gam, bet, 1e-5))

    gam, bet, ref = gn_ref(ya)
    one = ops.group_norm(ya, gam, bet, 32, 1e-5, silu=True)
    check(one, ref, BF, "gn tile partials")
    assert torch.equal(one, ops.group_norm(ya, gam, bet, 32, 1e-5, silu=True))
    gam, bet, ref = gn_ref(ya, yb)  # 960 channels, group size 30: groups straddle the two producers
    check(ops.group_norm(ya, gam, bet, 32, 1e-5, silu=True, x2=yb), ref, BF, "gn tile partials, concat")
    # a GEMM-produced image (32-row partials) next to a tile-partial one: per-producer granularity in the finalise kernel
    t = ops.linear(rnd(N * hw * hw, 64, seed=330).to(dev).to(BF).view(N, hw * hw, 64), rnd(320, 64, seed=331, scale=0.125).to(dev), None, gn_hw=hw * hw)
    yc = ops.image_of_stats(t, hw, hw)
    assert ops._gn_rows_of(yc) == 32 and ops._gn_stats_of(yc, hw * hw) is not None
    gam, bet, ref = gn_ref(yb, yc)
    check(ops.group_norm(yb, gam, bet, 32, 1e-5, silu=True, x2=yc), ref, BF, "gn tile + 32-row partials")
    gam, bet, ref = gn_ref(yc, ya)
    check(ops.group_norm(yc, gam, bet, 32, 1e-5, silu=True, x2=ya), ref, BF, "gn 32-row + tile partials")
    # the CFG prefix duplicates a tensor together with its statistics
    yd = ops.dup_batch(yb)
    assert ops._gn_rows_of(yd) == 256 and ops._gn_stats_of(yd, hw * hw) is not None
    gam, bet, ref = gn_ref(yb)
    got = ops.group_norm(yd, gam, bet, 32, 1e-5, silu=True)
    check(got[:N], ref, BF, "gn tile partials, dup (first half)")
    assert torch.equal(got[:N], got[N:])


@pytest.mark.parametrize("dtype", DTYPES)
def test_group_norm_concat(dtype):
    from cremage_amd import ops
    x1, x2 = rnd(2, 320, 6, 6, seed=53), rnd(2, 640, 6, 6, seed=54) * 2 + 1
    g, b = 1 + 0.1 * rnd(960, seed=55), 0.1 * rnd(960, seed=56)
    ref = F.silu(F.group_norm(torch.cat([q(x1, dtype), q(x2, dtype)], 1), 32, g, b, 1e-5))
    got = ops.group_norm(nhwc(x1, dtype), g.to(_dev()), b.to(_dev()), 32, 1e-5, silu=True, x2=nhwc(x2, dtype))
    check(got, ref, dtype, "group_norm concat")
    # single-launch path (group size 80, split on a group boundary)
    x1, x2 = rnd(2, 1280, 8, 8, seed=57) - 2, rnd(2, 1280, 8, 8, seed=58) * 3 + 1
    g, b = 1 + 0.1 * rnd(2560, seed=59), 0.1 * rnd(2560, seed=60)
    ref = F.silu(F.group_norm(torch.cat([q(x1, dtype), q(x2, dtype)], 1), 32, g, b, 1e-5))
    got = ops.group_norm(nhwc(x1, dtype), g.to(_dev()), b.to(_dev()), 32, 1e-5, silu=True, x2=nhwc(x2, dtype))
    check(got, ref, dtype, "group_norm concat (small)")


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("rows", [37, 8191, 20001])  # one row per wave / grid-stride steps of RW rows with an odd tail / > one sweep
@pytest.mark.parametrize("dim", [64, 320, 640, 1280, 2048])
def test_layer_norm(dtype, dim, rows):
    from cremage_amd import ops
    x = rnd(2, rows, dim, seed=60) + 0.5
    g, b = 1 + 0.1 * rnd(dim, seed=61), 0.1 * rnd(dim, seed=62)
    ref = F.layer_norm(q(x, dtype), (dim,), g, b, 1e-5)
    got = ops.layer_norm(x.to(_dev()).to(dtype), g.to(_dev()), b.to(_dev()), 1e-5)
    check(got, ref, dtype, "layer_norm")


def test_softmax_rows():
    from cremage_amd import ops
    x = rnd(3, 50, 80, seed=63, scale=3.0)
    got = ops.softmax_rows_(x.clone().to(_dev()), 77, 0.3)
    ref = torch.softmax(x[..., :77] * 0.3, dim=-1)
    check(got[..., :77], ref, torch.float32, "softmax_rows")


# ------------------------------------------------------------------------------------------ attention
def attn_ref(qq, kk, vv, heads, scale):
    B, Nq, C = qq.shape
    d = C // heads
    sp = lambda t: t.reshape(B, t.shape[1], heads, d).permute(0, 2, 1, 3)
    s = torch.einsum("bhid,bhjd->bhij", sp(qq), sp(kk)) * scale
    o = torch.einsum("bhij,bhjd->bhid", s.softmax(-1), sp(vv))
    return o.permute(0, 2, 1, 3).reshape(B, Nq, C)


@pytest.mark.parametrize("heads,d,Nq,Nk", [(8, 40, 200, 77), (8, 40, 256, 256), (8, 80, 100, 154), (8, 160, 64, 64), (2, 64, 130, 81),
                                           (4, 8, 33, 5), (4, 16, 64, 200), (2, 32, 700, 1000), (1, 128, 40, 90), (8, 40, 1024, 1024)])
def test_flash_attention(heads, d, Nq, Nk):
    from cremage_amd import ops
    C = heads * d
    qq, kk, vv = rnd(2, Nq, C, seed=70), rnd(2, Nk, C, seed=71), rnd(2, Nk, C, seed=72)
    ld = (Nk + 7) // 8 * 8
    vt = torch.zeros(2, C, ld)
    vt[:, :, :Nk] = vv.transpose(1, 2)
    vt[:, :, Nk:] = float("nan")  # pad columns must never leak into the result
    ref = attn_ref(q(qq, BF), q(kk, BF), q(vv, BF), heads, d ** -0.5)
    got = ops.attention(qq.to(_dev()).to(BF), kk.to(_dev()).to(BF), vt.to(_dev()).to(BF), heads, Nk, d ** -0.5)
    # P is rounded to bf16 before PV: allow the corresponding extra error
    got, ref = got.float().cpu(), ref
    rel = fig("attention rel-L2", ((got - ref).norm() / ref.norm()).item(), 1e-2 * HS)
    assert torch.isfinite(got).all() and rel < 1e-2 * HS, (rel, heads, d, Nq, Nk)


@pytest.mark.parametrize("heads,d,Nq,Nk", [(8, 40, 200, 77), (8, 40, 256, 256), (8, 80, 100, 154), (8, 160, 64, 64), (2, 64, 130, 81),
                                           (4, 8, 33, 5), (4, 16, 64, 200), (2, 32, 700, 1000), (1, 128, 40, 90), (8, 40, 1024, 1024),
                                           (20, 64, 300, 300), (8, 40, 128, 81)])
@pytest.mark.parametrize("fused", [False, True])
def test_flash_attention_row_major_v(heads, d, Nq, Nk, fused):
    """crg_attention_v: V row-major ([B, Nk, C], transposing LDS read inside the kernel).  `fused`: q / k / v are column slices of
    one [B, N, 3C] tensor (self-attention, Nq == Nk) or k / v slices of a [B, Nk, 2C] tensor (cross-attention) - the strided views
    the fused projections hand over - with NaNs in the neighbouring memory that must not leak."""
    from cremage_amd import ops
    C = heads * d
    qq, kk, vv = rnd(2, Nq, C, seed=170), rnd(2, Nk, C, seed=171), rnd(2, Nk, C, seed=172)
    ref = attn_ref(q(qq, BF), q(kk, BF), q(vv, BF), heads, d ** -0.5)
    dq, dk, dv = qq.to(_dev()).to(BF), kk.to(_dev()).to(BF), vv.to(_dev()).to(BF)
    if fused and Nq == Nk:
        qkv = torch.cat([dq, dk, dv], dim=-1)
        dq, dk, dv = qkv[..., :C], qkv[..., C:2 * C], qkv[..., 2 * C:]
    elif fused:
        kv = torch.cat([dk, dv], dim=-1)
        dk, dv = kv[..., :C], kv[..., C:]
    got = ops.attention_rows_v(dq, dk, dv, heads, d ** -0.5).float().cpu()
    rel = fig("attention rel-L2", ((got - ref).norm() / ref.norm()).item(), 1e-2 * HS)
    assert torch.isfinite(got).all() and rel < 1e-2 * HS, (rel, heads, d, Nq, Nk)


def test_flash_attention_row_major_v_spiky_rows():
    """the online-softmax rescale branch of the row-major-V variant (guide rule 26: force the branch)"""
    from cremage_amd import ops
    heads, d, Nq, Nk = 2, 64, 64, 300
    C = heads * d
    qq, kk, vv = rnd(1, Nq, C, seed=173), rnd(1, Nk, C, seed=174), rnd(1, Nk, C, seed=175)
    kk[0, 250] = qq[0, 3] * 4.0
    kk[0, 70] = qq[0, 9] * 6.0
    ref = attn_ref(q(qq, BF), q(kk, BF), q(vv, BF), heads, d ** -0.5)
    got = ops.attention_rows_v(qq.to(_dev()).to(BF), kk.to(_dev()).to(BF), vv.to(_dev()).to(BF), heads, d ** -0.5).float().cpu()
    assert fig("attention rel-L2", ((got - ref).norm() / ref.norm()).item(), 1e-2 * HS) < 1e-2 * HS


@pytest.mark.parametrize("heads,d,Nq,Nk", [(8, 40, 200, 192), (3, 48, 130, 64), (8, 40, 384, 1024), (2, 40, 128, 2048), (4, 64, 256, 256),
                                           (2, 64, 130, 192), (8, 80, 200, 128), (8, 80, 128, 320), (2, 80, 300, 1024)])
def test_flash_attention_lds_dma_form(heads, d, Nq, Nk):
    """attn_dma_kernel / attn_sp_kernel (whole 64-key tiles, K / V^T staged by LDS-DMA with the key permutation and the chunk swizzles;
    Nk % 128 == 0 takes the software-pipelined form, odd tile counts the plain one): q and k are column slices of a wider NaN-filled
    buffer (nothing outside the head's own channels may be read into a product), query tails, many key tiles (every stage reused),
    head dims 40 / 64 / 80 (each has its own K-image swizzle), and 48, which stays on the register-staged kernel."""
    from cremage_amd import ops
    C = heads * d
    qq, kk, vv = rnd(2, Nq, C, seed=270), rnd(2, Nk, C, seed=271), rnd(2, Nk, C, seed=272)
    kk[1, Nk - 3] = qq[1, 5] * 5.0  # a late dominant key: the rescale branch
    ref = attn_ref(q(qq, BF), q(kk, BF), q(vv, BF), heads, d ** -0.5)
    wide_q = torch.full((2, Nq, C + 16), float("nan"))
    wide_k = torch.full((2, Nk, C + 24), float("nan"))
    wide_q[..., 8:8 + C] = qq
    wide_k[..., 8:8 + C] = kk
    dq = wide_q.to(_dev()).to(BF)[..., 8:8 + C]
    dk = wide_k.to(_dev()).to(BF)[..., 8:8 + C]
    vt = vv.transpose(1, 2).contiguous().to(_dev()).to(BF)
    got = ops.attention(dq, dk, vt, heads, Nk, d ** -0.5).float().cpu()
    rel = fig("attention rel-L2", ((got - ref).norm() / ref.norm()).item(), 1e-2 * HS)
    assert torch.isfinite(got).all() and rel < 1e-2 * HS, (rel, heads, d, Nq, Nk)


@pytest.mark.parametrize("heads,d,Nq,Nk,row_major_v", [(8, 40, 2100, 77, False), (8, 40, 2100, 77, True), (8, 40, 2048, 4, False), (8, 40, 2048, 4, True),
                                                       (8, 64, 2100, 64, True), (8, 64, 2050, 128, False), (8, 80, 2100, 81, False), (8, 80, 2100, 81, True),
                                                       (8, 160, 2064, 77, True), (16, 8, 1100, 5, False), (8, 48, 2100, 100, False), (8, 128, 2100, 96, True)])
def test_flash_attention_few_keys_kernel(heads, d, Nq, Nk, row_major_v):
    """attn_ctx_kernel (Nk <= 128 and ceil(Nq / 128) * B * H >= 2048 blocks' worth of query groups: the 64x64-level cross-attention
    against the prompt context, FaceID's 4 tokens): both key tiles staged once per block, the block then walks several 128-query groups
    with the next group's Q fragments requested ahead.  B = 16 reaches the dispatch threshold; one and two key tiles, key tails (77, 81,
    4, 5, 100), a query tail in the last group, every head-dim family (k-steps 1, 3, 4, 5, 8, 10 incl. the all-ones denominator variants),
    transposed V (crg_attention, NaN pad columns) and row-major V (crg_attention_v: k / v column slices of one NaN-guarded buffer)."""
    from cremage_amd import ops
    B = 16
    assert (Nq + 127) // 128 * B * heads >= 2048 and Nk <= 128  # the dispatch rule of attention_entry (attention.hip)
    C = heads * d
    qq, kk, vv = rnd(B, Nq, C, seed=470), rnd(B, Nk, C, seed=471), rnd(B, Nk, C, seed=472)
    kk[3, Nk - 1] = qq[3, 7, :].clone() * 3.0  # a dominant last key (inside the tail tile)
    ref = attn_ref(q(qq, BF), q(kk, BF), q(vv, BF), heads, d ** -0.5)
    wide_q = torch.full((B, Nq, C + 16), float("nan"))
    wide_q[..., 8:8 + C] = qq
    dq = wide_q.to(_dev()).to(BF)[..., 8:8 + C]
    if row_major_v:
        kv = torch.full((B, Nk, 2 * C + 24), float("nan"))
        kv[..., 8:8 + C] = kk
        kv[..., 16 + C:16 + 2 * C] = vv
        kv = kv.to(_dev()).to(BF)
        got = ops.attention_rows_v(dq, kv[..., 8:8 + C], kv[..., 16 + C:16 + 2 * C], heads, d ** -0.5)
    else:
        ld = (Nk + 7) // 8 * 8
        vt = torch.full((B, C, ld), float("nan"))
        vt[:, :, :Nk] = vv.transpose(1, 2)
        got = ops.attention(dq, kk.to(_dev()).to(BF), vt.to(_dev()).to(BF), heads, Nk, d ** -0.5)
    got = got.float().cpu()
    rel = fig("attention rel-L2", ((got - ref).norm() / ref.norm()).item(), 1e-2 * HS)
    worst = ((got - ref).flatten(1).norm(dim=1) / ref.flatten(1).norm(dim=1)).max().item()  # per sample: a wrong group cannot hide in the norm
    assert torch.isfinite(got).all() and rel < 1e-2 * HS and worst < 1.5e-2 * HS, (rel, worst, heads, d, Nq, Nk)


@pytest.mark.parametrize("gain", [30.0, 300.0])
def test_flash_attention_large_logits(gain):
    """the pipelined kernel keeps the softmax shift INSIDE the MFMA (channels 40, 41 of Q against ones in K) and moves it lazily:
    logits in the hundreds / tens of thousands (softmax ~ one-hot, the reference moving by thousands between tiles, negative row
    maxima) must neither overflow nor lose the row"""
    from cremage_amd import ops
    heads, d, Nq, Nk = 8, 40, 256, 512
    C = heads * d
    qq, kk, vv = rnd(1, Nq, C, seed=370) * gain, rnd(1, Nk, C, seed=371), rnd(1, Nk, C, seed=372)
    kk[0, 300:] *= 3.0          # larger logits late: the reference has to move after the first tiles
    qq[0, :16] = -qq[0, :16].abs()  # rows whose logits against the positive keys below are all negative
    kk[0, :64] = kk[0, :64].abs()
    ref = attn_ref(q(qq, BF), q(kk, BF), q(vv, BF), heads, d ** -0.5)
    vt = vv.transpose(1, 2).contiguous().to(_dev()).to(BF)
    got = ops.attention(qq.to(_dev()).to(BF), kk.to(_dev()).to(BF), vt, heads, Nk, d ** -0.5).float().cpu()
    assert torch.isfinite(got).all()
    # a near-one-hot softmax amplifies the bf16 rounding of Q * scale * log2(e) (the winner can change between two close keys):
    # compare where the reference softmax is decisive, and bound the rest loosely
    rel = fig("attention rel-L2", ((got - ref).norm() / ref.norm()).item(), (2e-2 if gain < 100 else 2e-1) * HS)
    assert rel < (2e-2 if gain < 100 else 2e-1) * HS, (gain, rel)


def test_flash_attention_spiky_rows():
    """online-softmax rescale path: one key dominates late in the sequence (guide rule 26)"""
    from cremage_amd import ops
    heads, d, Nq, Nk = 2, 64, 64, 300
    C = heads * d
    qq, kk, vv = rnd(1, Nq, C, seed=73), rnd(1, Nk, C, seed=74), rnd(1, Nk, C, seed=75)
    kk[0, 250] = qq[0, 3] * 4.0   # query 3 (and correlated rows) jump to a new max at key tile 3
    kk[0, 70] = qq[0, 9] * 6.0
    vt = vv.transpose(1, 2).contiguous()
    vt = F.pad(vt, (0, (-Nk) % 8))
    ref = attn_ref(q(qq, BF), q(kk, BF), q(vv, BF), heads, d ** -0.5)
    got = ops.attention(qq.to(_dev()).to(BF), kk.to(_dev()).to(BF), vt.to(_dev()).to(BF), heads, Nk, d ** -0.5).float().cpu()
    assert fig("attention rel-L2", ((got - ref).norm() / ref.norm()).item(), 1e-2 * HS) < 1e-2 * HS


@pytest.mark.parametrize("dtype,heads,d", [(torch.float32, 4, 32), (torch.float32, 8, 40), (BF, 1, 512), (torch.float32, 1, 512)])
def test_unfused_attention(dtype, heads, d):
    from cremage_amd import ops
    C, Nq, Nk = heads * d, 70, 77
    qq, kk, vv = rnd(2, Nq, C, seed=76), rnd(2, Nk, C, seed=77), rnd(2, Nk, C, seed=78)
    vt = F.pad(vv.transpose(1, 2), (0, (-Nk) % 8)).contiguous()
    ref = attn_ref(q(qq, dtype), q(kk, dtype), q(vv, dtype), heads, d ** -0.5)
    got = ops.attention(qq.to(_dev()).to(dtype), kk.to(_dev()).to(dtype), vt.to(_dev()).to(dtype), heads, Nk, d ** -0.5).float().cpu()
    rel = fig("attention rel-L2", ((got - ref).norm() / ref.norm()).item(), 1e-2 * HS if dtype == BF else 5e-5)
    assert rel < (1e-2 * HS if dtype == BF else 5e-5), rel


@pytest.mark.parametrize("dtype,heads,d", [(BF, 1, 512), (torch.float32, 1, 512), (torch.float32, 4, 32)])
def test_unfused_attention_query_chunks_with_tail(dtype, heads, d, monkeypatch):
    """The chunked unfused path with SEVERAL query chunks plus a shorter last one and a padded key count (kp != n_keys): the
    branch the VAE AttnBlock takes at 768x768 (9216 tokens: chunks of 7280 + a tail of 1936).  The score budget is shrunk so that
    a small case walks the same code: Nq = 150 in chunks of 64 -> 64, 64, 22."""
    from cremage_amd import ops
    C, Nq, Nk = heads * d, 150, 77
    kp = (Nk + 7) // 8 * 8
    monkeypatch.setattr(ops.knobs, "SCORE_BUDGET_BYTES", 4 * heads * kp * 64)
    qq, kk, vv = rnd(2, Nq, C, seed=86), rnd(2, Nk, C, seed=87), rnd(2, Nk, C, seed=88)
    vt = F.pad(vv.transpose(1, 2), (0, (-Nk) % 8)).contiguous()
    ref = attn_ref(q(qq, dtype), q(kk, dtype), q(vv, dtype), heads, d ** -0.5)
    got = ops.attention(qq.to(_dev()).to(dtype), kk.to(_dev()).to(dtype), vt.to(_dev()).to(dtype), heads, Nk, d ** -0.5).float().cpu()
    rel = fig("attention rel-L2", ((got - ref).norm() / ref.norm()).item(), 1e-2 * HS if dtype == BF else 5e-5)
    assert rel < (1e-2 * HS if dtype == BF else 5e-5), rel


# ------------------------------------------------------------------------------------------ small ops
def test_timestep_embedding_kernel(golden):
    from cremage_amd import ops
    meta, g = golden("op_timestep_embedding")
    got = ops.timestep_embedding(g["t"].to(_dev()), 320).cpu()
    assert (got - g["e320"]).abs().max().item() < 2e-4  # sin/cos of args up to ~1e3 rad: 1 ulp of the argument
    got = ops.timestep_embedding(g["t"].to(_dev()), 64).cpu()
    assert (got - g["e64"]).abs().max().item() < 2e-4


@pytest.mark.parametrize("dtype", DTYPES)
def test_layout_and_elementwise(dtype):
    from cremage_amd import ops
    x = rnd(2, 5, 7, 9, seed=80)
    y = ops.nchw_to_nhwc(x.to(_dev()), dtype)
    assert y.shape == x.shape and y.permute(0, 2, 3, 1).is_contiguous()
    check(y, q(x, dtype), torch.float32, "nchw_to_nhwc")
    z = ops.nhwc_to_nchw(y, torch.float32)
    assert z.is_contiguous()
    check(z, q(x, dtype), torch.float32, "nhwc_to_nchw")
    s = ops.silu(x.to(_dev()).to(dtype))
    check(s, F.silu(q(x, dtype)), dtype, "silu")
    a = ops.affine_cast(x.to(_dev()), 0.5, 0.5, torch.float32, 0.0, 1.0)
    check(a, (x * 0.5 + 0.5).clamp(0, 1), torch.float32, "affine_cast")
    yy = x.to(_dev()).to(dtype).clone()
    ops.axpby_(yy, (2 * x).to(_dev()).to(dtype), 0.25, 1.0)
    check(yy, q(x, dtype) + 0.25 * q(2 * x, dtype), dtype, "axpby")


def test_errors_are_python_exceptions():
    """the library never aborts: bad arguments come back as CrgError (mp/mp.py:125 has no handler)"""
    from cremage_amd import _lib as L
    from cremage_amd import ops
    with pytest.raises(L.CrgError):
        ops.linear(torch.zeros(4, 12, device=_dev(), dtype=BF), torch.zeros(8, 12, device=_dev()))  # K % 8 != 0
    with pytest.raises(L.CrgError):
        ops.linear(torch.zeros(4, 16), torch.zeros(8, 16))  # CPU tensors: no fallback
    with pytest.raises(L.CrgError):
        ops.group_norm(torch.zeros(1, 36, 4, 4, device=_dev(), dtype=BF), torch.ones(36, device=_dev()), torch.zeros(36, device=_dev()), 32, 1e-5)


def test_cfg_euler_step_matches_the_elementwise_chain():
    """crg_cfg_euler_step == CompVisDenoiser scalings + CFG + Euler(-ancestral) update written as separate fp32 ops
    (external.py:111-114, ldm_wrapper_for_k_diffusion.py:99, sampling.py:134-142,157-162), one rounding at a time"""
    from cremage_amd import ops
    b, shape = 3, (4, 16, 16)
    x = rnd(b, *shape, seed=90).to(_dev())
    eps = rnd(2 * b, *shape, seed=91).to(_dev())
    noise = rnd(b, *shape, seed=92).to(_dev())
    sigma, dt, cfg, nscale = 3.7, -0.9, 7.5, 0.35
    for nz in (None, noise):
        e_u, e_c = eps.chunk(2)
        den_u, den_c = x + e_u * (-sigma), x + e_c * (-sigma)
        den = den_u + cfg * (den_c - den_u)
        ref = x + ((x - den) / sigma) * dt
        if nz is not None:
            ref = ref + nz * nscale
        got = ops.cfg_euler_step_(x.clone(), eps, nz, sigma, dt, cfg, nscale)
        assert (got - ref).abs().max().item() <= 2e-6 * max(1.0, ref.abs().max().item())
