"""Kernel-level parity of the batched, strided crg_gemm (batch > 1, a_bstride / w_bstride / y_bstride / r_bstride, ldy != N) and of the row
softmax between its two uses: the path of `ops.attention`'s unfused branch (every fp32 attention, the VAE AttnBlock) and of
`ops.linear_transposed`.  The whole-network goldens reach these shapes with a whole network's tolerance; here every branch of
the GEMM planner's split-K choice (gemm_plan.h), gemm_conv.hip's launcher and splitk_reduce.hip's `splitk_reduce_kernel` that a batch can reach is compared on its own:

  A  raw crg_gemm through `ops._gemm` (the ctypes struct the wrappers fill) with explicit strides, on buffers LARGER than the operands:
     what belongs to no operand holds NaN on the input side and a sentinel on the output side, which must survive bitwise
  B  ops.linear_transposed (weight as the A operand, BIAS_ROW, batch = B), both activation dtypes
  C  ops.attention on the unfused branch: global and per (sample, head) rel-L2, the pad-column contract
  D  ops.softmax_rows_ in fp32 and in the half type, in place, with sentinel pad columns

Generic over the process's half type exactly as tests/test_hip_ops.py (BF, HS; tests/test_hip_ops_f16.py runs this file against the
fp16 library).  References are fp64 on the operands as the kernel sees them (rounded with q(.., BF) wherever the kernel reads or
stages the half type; the fp32-class path sees the unrounded fp32 operands).  Bounds are check()'s, and 1e-2 * HS / 5e-5 rel-L2 for
attention as in test_unfused_attention.

Which kernel ran is asserted, not assumed: every case states the profiler slots (one per kernel family and tile width, and the
split-K reduce) it must launch, so a shape that stops reaching its branch fails.  The tile configuration (C / D / A) has no slot of
its own: the figures in the tables below are `launch`'s arithmetic on 128-row tiles (blocks = tiles * batch: < 192 -> C, < 384 -> D,
else A; a K cut always runs on A).
"""
import pytest
import torch
import torch.nn.functional as F

from tests.test_hip_ops import BF, HS, _dev, check, fig, q, rnd

pytestmark = pytest.mark.gpu

F32 = torch.float32
SENTINEL = -1024.0  # exact in bf16, fp16 and fp32
GUARD = 64          # elements in front of every buffer that belong to no operand (keeps the operand 16-byte aligned)
NAN = float("nan")


def _launches(pr):
    return {k: v["launches"] for k, v in pr.kernels.items() if v["launches"]}


# ------------------------------------------------------------------------------------------ A: raw batched crg_gemm
def _buffer(data, bs, ld, dtype, fill, tail):
    """flat device buffer, `fill` everywhere except the [batch][rows][cols] operand laid out with strides (bs, ld, 1) behind GUARD
    elements; `tail` more elements follow the operand's last one (rows past M / N of the last batch)"""
    b, r, c = data.shape
    host = torch.full((GUARD + (b - 1) * bs + (r - 1) * ld + c + tail,), fill, dtype=F32)
    host.as_strided((b, r, c), (bs, ld, 1), GUARD).copy_(data)
    return host.to(_dev()).to(dtype)


def _view(buf, shape, bs, ld):
    return buf.cpu().as_strided(shape, (bs, ld, 1), GUARD)


def _ptr(buf):
    return buf.data_ptr() + GUARD * buf.element_size()


def _raw_gemm(*, a_dtype, y_dtype, x3, batch, M, N, K, lda, a_bs, ldw, w_bs, ldy, y_bs, ldr=0, r_bs=0, bias=False, silu=False,
              a_zero_cols=0, seed=500, expect=None, what=""):
    """one crg_gemm call with explicit strides; asserts the sentinel outside (b < batch, m < M, n < N), check()s the inside against
    the fp64 reference built from as_strided views of the SAME device buffers, and asserts the kernel slots that ran"""
    from cremage_amd import _lib as L
    from cremage_amd import ops
    a = rnd(batch, M, K, seed=seed)
    w = rnd(batch, N, K, seed=seed + 1, scale=K ** -0.5)
    if a_zero_cols:  # the score pad columns of the PV GEMM: zeros in A against finite values in W
        a[:, :, K - a_zero_cols:] = 0
    A = _buffer(a, a_bs, lda, a_dtype, NAN, 2 * lda + GUARD)
    if x3:
        wh = w.to(BF)
        W = _buffer(wh.float(), w_bs, ldw, BF, NAN, 2 * ldw + GUARD)
        Wlo = _buffer((w - wh.float()).to(BF).float(), w_bs, ldw, BF, NAN, 2 * ldw + GUARD)
    else:
        W, Wlo = _buffer(w, w_bs, ldw, BF, NAN, 2 * ldw + GUARD), None
    Y = _buffer(torch.full((batch, M, N), SENTINEL), y_bs, ldy, y_dtype, SENTINEL, 2 * ldy + GUARD)
    R = _buffer(rnd(batch, M, N, seed=seed + 2), r_bs, ldr, y_dtype, NAN, 2 * ldr + GUARD) if ldr else None
    bvec = rnd(N, seed=seed + 3).to(_dev()) if bias else None

    # the reference: fp64 on what the kernel sees
    ra = _view(A, (batch, M, K), a_bs, lda).double()
    if a_dtype == F32 and not x3:
        ra = q(ra.float(), BF).double()  # P is rounded to the half type while it is staged
    rw = w.double() if x3 else _view(W, (batch, N, K), w_bs, ldw).double()
    ref = torch.einsum("bmk,bnk->bmn", ra, rw)
    if bias:
        ref = ref + bvec.cpu().double()
    if silu:
        ref = F.silu(ref)
    if R is not None:
        ref = ref + _view(R, (batch, M, N), r_bs, ldr).double()

    h = ops._h(A)
    with ops.profile() as pr:
        ops._gemm(h, a=_ptr(A), lda=lda, a_bstride=a_bs, w=_ptr(W), ldw=ldw, w_bstride=w_bs, w_lo=_ptr(Wlo) if x3 else None,
                  bias=bvec.data_ptr() if bias else None, bias_mode=L.BIAS_COL if bias else L.BIAS_NONE,
                  residual=_ptr(R) if R is not None else None, ldr=ldr, r_bstride=r_bs, y=_ptr(Y), ldy=ldy, y_bstride=y_bs,
                  M=M, N=N, K=K, batch=batch, epilogue=L.EPI_SILU if silu else L.EPI_NONE,
                  a_dtype=L.F32 if a_dtype == F32 else L.BF16, y_dtype=L.F32 if y_dtype == F32 else L.BF16,
                  prec=L.PREC_BF16X3 if x3 else L.PREC_BF16, a_is_weight=0, a_lo=None)
    ran = _launches(pr)
    print(f"[ran] {what}: {ran}")

    inside = torch.zeros(Y.numel(), dtype=torch.bool)
    inside.as_strided((batch, M, N), (y_bs, ldy, 1), GUARD).fill_(True)
    out = Y.cpu()
    sent = torch.full((1,), SENTINEL, dtype=y_dtype)
    ibits = torch.int16 if y_dtype != F32 else torch.int32
    touched = (out.view(ibits) != sent.view(ibits)) & ~inside
    assert not touched.any(), (what, "wrote outside its operand at flat offsets", (touched.nonzero().flatten() - GUARD)[:8].tolist())
    # BF bound where the output or the staged A is rounded to the half type; fp32-class bound for fp32 outputs of exact operands
    bound = BF if (y_dtype != F32) else F32
    check(_view(Y, (batch, M, N), y_bs, ldy), ref, bound, what)
    assert ran == expect, (what, ran, expect)


# case -> (arguments, slots that must run).  Tiles on 128-row tiles; k-tiles of 64.
RAW = {
    # one head-interleaved [M][heads * K] buffer with 8 NaN columns behind the heads; 2 x 1 tiles x 3 = 6 blocks -> C; N & 3 != 0;
    # K = 40 is less than one k-tile; the score buffer's head stride covers 208 rows (a longer chunk's) with ldy = roundup(N, 8)
    "score-C": (dict(a_dtype=BF, y_dtype=F32, x3=False, batch=3, M=200, N=77, K=40, lda=128, a_bs=40, ldw=128, w_bs=40, ldy=80, y_bs=208 * 80),
                {"gemm_w4": 1}),
    # 12 x 2 tiles x 8 heads = 192 blocks -> D (64-row tiles, 4 waves)
    "score-D": (dict(a_dtype=BF, y_dtype=F32, x3=False, batch=8, M=1536, N=200, K=40, lda=328, a_bs=40, ldw=328, w_bs=40, ldy=200, y_bs=1536 * 200),
                {"gemm_w4": 1}),
    # 24 x 2 x 8 = 384 blocks -> A (128-row tiles, two blocks per CU)
    "score-A": (dict(a_dtype=BF, y_dtype=F32, x3=False, batch=8, M=3072, N=200, K=40, lda=328, a_bs=40, ldw=328, w_bs=40, ldy=200, y_bs=3072 * 200),
                {"gemm_w4": 1}),
    # N % 160 == 0: 160-wide tiles (2 x 2 x 2 = 8 blocks, C)
    "score-W5-f32": (dict(a_dtype=BF, y_dtype=F32, x3=False, batch=2, M=130, N=320, K=160, lda=168, a_bs=136 * 168, ldw=168, w_bs=328 * 168,
                          ldy=328, y_bs=136 * 328), {"gemm_w5": 1}),
    # ... and the paired (16-byte) epilogue of a half output: N, ldy and y_bs multiples of 8
    "score-W5-half": (dict(a_dtype=BF, y_dtype=BF, x3=False, batch=2, M=130, N=320, K=160, lda=168, a_bs=136 * 168, ldw=168, w_bs=328 * 168,
                           ldy=328, y_bs=136 * 328), {"gemm_w5": 1}),
    # N <= 32: the 32-wide tile
    "score-W1": (dict(a_dtype=BF, y_dtype=F32, x3=False, batch=4, M=300, N=16, K=64, lda=264, a_bs=64, ldw=264, w_bs=64, ldy=24, y_bs=304 * 24),
                 {"gemm_w1": 1}),
    # 2 tiles x 4 = 8 blocks, 24 k-tiles -> 3 K slices: slab offset per batch, reduce into a head-interleaved y (ldy 160, y_bs 40)
    "splitk-batch-f32": (dict(a_dtype=BF, y_dtype=F32, x3=False, batch=4, M=200, N=40, K=1536, lda=4 * 1536 + 8, a_bs=1536, ldw=4 * 1536 + 8,
                              w_bs=1536, ldy=160, y_bs=40), {"gemm_w4": 1, "splitk_reduce": 1}),
    "splitk-batch-half": (dict(a_dtype=BF, y_dtype=BF, x3=False, batch=4, M=200, N=40, K=1536, lda=4 * 1536 + 8, a_bs=1536, ldw=4 * 1536 + 8,
                               w_bs=1536, ldy=160, y_bs=40), {"gemm_w4": 1, "splitk_reduce": 1}),
    # the PV GEMM: fp32 A (probabilities, rounded to the half type while staged) on the register-staged kernel, 3 x 8 = 24 blocks,
    # 3 K slices, A's head stride covers 304 rows, output interleaved by head
    "pv-split": (dict(a_dtype=F32, y_dtype=BF, x3=False, batch=8, M=300, N=40, K=1536, lda=1536, a_bs=304 * 1536, ldw=1536, w_bs=40 * 1536,
                      ldy=320, y_bs=40), {"gemm_x3": 1, "splitk_reduce": 1}),
    # ... unsplit, with the pad columns 77..79 of A zero against finite values in W
    "pv-short": (dict(a_dtype=F32, y_dtype=BF, x3=False, batch=8, M=300, N=40, K=80, lda=80, a_bs=304 * 80, ldw=80, w_bs=40 * 80, ldy=320, y_bs=40,
                      a_zero_cols=3), {"gemm_x3": 1}),
    # fp32-class (hi * hi + hi * lo + lo * hi) from fp32 A: unsplit on the score-C shape, batched K split on the pv-split shape
    "x3-score": (dict(a_dtype=F32, y_dtype=F32, x3=True, batch=3, M=200, N=77, K=40, lda=128, a_bs=40, ldw=128, w_bs=40, ldy=80, y_bs=208 * 80),
                 {"gemm_x3": 1}),
    "x3-pv": (dict(a_dtype=F32, y_dtype=F32, x3=True, batch=8, M=300, N=40, K=1536, lda=1536, a_bs=304 * 1536, ldw=1536, w_bs=40 * 1536, ldy=320,
                   y_bs=40), {"gemm_x3": 1, "splitk_reduce": 1}),
    # residual with its own batch stride + BIAS_COL (+ SiLU) with a batch: in the split-K reduce (K = 1536, 3 slices) and in the
    # epilogue of the unsplit kernel (K = 128): ldr = 100 keeps the 4-wide epilogue, ldr = 104 / r_bs % 8 == 0 takes the paired one
    "epi-batch-reduce": (dict(a_dtype=BF, y_dtype=BF, x3=False, batch=2, M=200, N=96, K=1536, lda=1544, a_bs=203 * 1544, ldw=1544, w_bs=99 * 1544,
                              ldy=104, y_bs=208 * 104, ldr=100, r_bs=203 * 100, bias=True), {"gemm_w4": 1, "splitk_reduce": 1}),
    "epi-batch-reduce-silu": (dict(a_dtype=BF, y_dtype=BF, x3=False, batch=2, M=200, N=96, K=1536, lda=1544, a_bs=203 * 1544, ldw=1544,
                                   w_bs=99 * 1544, ldy=104, y_bs=208 * 104, ldr=100, r_bs=203 * 100, bias=True, silu=True),
                              {"gemm_w4": 1, "splitk_reduce": 1}),
    "epi-batch-plain": (dict(a_dtype=BF, y_dtype=BF, x3=False, batch=2, M=200, N=96, K=128, lda=136, a_bs=203 * 136, ldw=136, w_bs=99 * 136,
                             ldy=104, y_bs=208 * 104, ldr=100, r_bs=203 * 100, bias=True), {"gemm_w4": 1}),
    "epi-batch-paired-silu": (dict(a_dtype=BF, y_dtype=BF, x3=False, batch=2, M=200, N=96, K=128, lda=136, a_bs=203 * 136, ldw=136, w_bs=99 * 136,
                                   ldy=104, y_bs=208 * 104, ldr=104, r_bs=208 * 104, bias=True, silu=True), {"gemm_w4": 1}),
}


@pytest.mark.parametrize("case", list(RAW))
def test_raw_batched_gemm(case):
    kw, expect = RAW[case]
    _raw_gemm(expect=expect, what=case, seed=500 + 10 * list(RAW).index(case), **kw)


# ------------------------------------------------------------------------------------------ B: linear_transposed
@pytest.mark.parametrize("dtype", [BF, F32])
@pytest.mark.parametrize("B,T,K,N,bias,reduces", [
    (2, 80, 1536, 128, True, 1),    # 1 tile x 2, 24 k-tiles -> 3 slices: BIAS_ROW in the reduce, batch; fp32: a_is_weight with a_lo
    (3, 1000, 320, 320, True, 0),   # 8 n-tiles with a ragged last one x 3 m-tiles x 3 = 72 blocks -> C
    (16, 520, 320, 320, True, 0),   # 5 x 3 x 16 = 240 blocks -> D
    (2, 16, 2048, 640, False, 1),   # N <= 32 (the 32-wide tile), 5 x 2 = 10 blocks, 32 k-tiles -> 4 slices
    (2, 77, 2048, 640, True, 0)])   # a long K that must NOT split: N & 3 != 0 (the slab is read 4 columns at a time)
def test_linear_transposed_batched(dtype, B, T, K, N, bias, reduces):
    from cremage_amd import ops
    x, w, b = rnd(B, T, K, seed=520), rnd(N, K, seed=521, scale=K ** -0.5), rnd(N, seed=522) if bias else None
    ref = F.linear(q(x, dtype).double(), (q(w, BF) if dtype == BF else w).double(), b.double() if bias else None).transpose(1, 2)
    dx, dw, db = x.to(_dev()).to(dtype), w.to(_dev()), b.to(_dev()) if bias else None
    ops.packed_weight(dw, 0, dtype == F32)  # pack outside the profile: only the GEMM's own launches are counted
    with ops.profile() as pr:
        got = ops.linear_transposed(dx, dw, db)
    ran = _launches(pr)
    print(f"[ran] linear_transposed {B}x{T}x{K}x{N}: {ran}")
    ld = (T + 7) // 8 * 8
    assert got.shape == (B, N, ld) and got.dtype == dtype
    check(got[:, :, :T], ref, dtype, f"linear_transposed {B}x{T}x{K}x{N}")
    assert (got[:, :, T:] == 0).all()
    slot = "gemm_x3" if dtype == F32 else ("gemm_w1" if T <= 32 else "gemm_w4")  # (no T here is a multiple of 160)
    assert ran.get(slot) == 1 and ran.get("splitk_reduce", 0) == reduces, ran


# ------------------------------------------------------------------------------------------ C: unfused attention
def _attn_ref64(qq, kk, vv, heads, scale):
    B, Nq, C = qq.shape
    d = C // heads
    sp = lambda t: t.double().reshape(B, t.shape[1], heads, d).permute(0, 2, 1, 3)
    s = torch.einsum("bhid,bhjd->bhij", sp(qq), sp(kk)) * scale
    o = torch.einsum("bhij,bhjd->bhid", s.softmax(-1), sp(vv))
    return o.permute(0, 2, 1, 3).reshape(B, Nq, C)


def _attn_inputs(dtype, B, heads, d, Nq, Nk, late_key):
    C = heads * d
    qq, kk, vv = rnd(B, Nq, C, seed=530), rnd(B, Nk, C, seed=531), rnd(B, Nk, C, seed=532)
    if late_key:
        kk[0, Nk - 3] = qq[0, 5] * 5  # one dominant key three from the end (inside the ragged last score tile)
    vt = F.pad(vv.transpose(1, 2), (0, (-Nk) % 8)).contiguous()
    return qq, kk, vv, vt


@pytest.mark.parametrize("dtype,B,heads,d,Nq,Nk,late_key,chunk,reduces", [
    (F32, 2, 8, 40, 300, 1536, False, None, 2),  # PV: 3 tiles x 8 heads, 24 k-tiles -> 3 slices with batch 8, once per sample
    (F32, 2, 8, 40, 300, 1531, True, None, 2),   # kp != Nk: ragged score tiles (N & 3 != 0: unsplit), PV over kp = 1536
    (F32, 2, 4, 160, 200, 320, False, None, 0),  # 160-wide tiles in both GEMMs
    (F32, 1, 1, 512, 200, 1536, True, None, 1),  # the VAE AttnBlock forms: one head of 512 channels; PV 4 x 2 tiles -> 3 slices
    (BF, 1, 1, 512, 200, 1536, True, None, 1),
    (F32, 2, 8, 40, 300, 1536, False, 128, 6)])  # chunks of 128, 128 and 44 queries, each with a K-split PV GEMM
def test_unfused_attention_batched(dtype, B, heads, d, Nq, Nk, late_key, chunk, reduces, monkeypatch):
    from cremage_amd import ops
    assert dtype == F32 or d > 160  # the unfused branch of ops.attention
    if chunk:
        monkeypatch.setattr(ops.knobs, "SCORE_BUDGET_BYTES", 4 * heads * ((Nk + 7) // 8 * 8) * chunk)
    qq, kk, vv, vt = _attn_inputs(dtype, B, heads, d, Nq, Nk, late_key)
    ref = _attn_ref64(q(qq, dtype), q(kk, dtype), q(vv, dtype), heads, d ** -0.5)
    with ops.profile() as pr:
        got = ops.attention(qq.to(_dev()).to(dtype), kk.to(_dev()).to(dtype), vt.to(_dev()).to(dtype), heads, Nk, d ** -0.5)
    ran = _launches(pr)
    print(f"[ran] attention {B}x{heads}x{d} {Nq}x{Nk}: {ran}")
    got = got.double().cpu()
    bound = 1e-2 * HS if dtype == BF else 5e-5
    rel = fig("attention rel-L2", ((got - ref).norm() / ref.norm()).item(), bound)
    per = lambda t: t.reshape(B, Nq, heads, d).permute(0, 2, 1, 3).flatten(2).norm(dim=2)  # [sample][head]
    worst = fig("attention worst (sample, head) rel-L2", (per(got - ref) / per(ref)).max().item(), 1.5 * bound)
    assert torch.isfinite(got).all() and rel < bound and worst < 1.5 * bound, (rel, worst)
    chunks = B * (1 if not chunk else -(-Nq // chunk))
    # per chunk: the PV GEMM on the register-staged kernel (fp32 A), and the fp32-class score GEMM too; the half-type score GEMM on the
    # LDS-DMA kernel; never the flash kernel
    want = {"gemm_x3": 2 * chunks} if dtype == F32 else {"gemm_x3": chunks, "gemm_w4": chunks}
    assert ran.get("splitk_reduce", 0) == reduces and "attention" not in ran and all(ran.get(k) == v for k, v in want.items()), ran


def test_unfused_attention_finite_garbage_in_v_pads():
    """The unfused branch multiplies V^T's pad columns by the score pad columns instead of masking them: those are exact zeros (the
    score GEMM and the softmax write columns < n_keys only), so FINITE garbage in V^T's pads must give bitwise the output of zero pads."""
    from cremage_amd import ops
    heads, d, Nq, Nk = 1, 512, 200, 1531
    qq, kk, vv, vt = _attn_inputs(BF, 1, heads, d, Nq, Nk, True)
    assert vt.shape[-1] == 1536
    garbage = vt.clone()
    garbage[:, :, Nk:] = 6e4  # finite in bf16 and in fp16
    dq, dk = qq.to(_dev()).to(BF), kk.to(_dev()).to(BF)
    clean = ops.attention(dq, dk, vt.to(_dev()).to(BF), heads, Nk, d ** -0.5)
    dirty = ops.attention(dq, dk, garbage.to(_dev()).to(BF), heads, Nk, d ** -0.5)
    assert torch.isfinite(dirty.float()).all()
    assert torch.equal(clean, dirty)
    ref = _attn_ref64(q(qq, BF), q(kk, BF), q(vv, BF), heads, d ** -0.5)
    rel = fig("attention rel-L2", ((dirty.double().cpu() - ref).norm() / ref.norm()).item(), 1e-2 * HS)
    assert rel < 1e-2 * HS, rel


# ------------------------------------------------------------------------------------------ D: softmax_rows_
@pytest.mark.parametrize("dtype", [F32, BF])
@pytest.mark.parametrize("cols", [1, 7, 77, 256, 257, 4099])  # one column; < a wave; the score width; the block's 256 threads +- 1; many sweeps
def test_softmax_rows_strided(dtype, cols):
    """in place on rows of stride ld = roundup(cols, 8) + 8 whose pad columns hold a sentinel: fp64 softmax of the STORED input"""
    from cremage_amd import ops
    ld = (cols + 7) // 8 * 8 + 8
    g = torch.Generator().manual_seed(540 + cols)

    def run(rows, scale, what):
        host = torch.full((rows.shape[0], ld), SENTINEL)
        host[:, :cols] = rows
        x = host.to(_dev()).to(dtype)
        stored = x.cpu()
        ref = torch.softmax(stored[:, :cols].double() * scale, dim=-1)
        out = ops.softmax_rows_(x, cols, scale)
        assert out.data_ptr() == x.data_ptr()
        got = x.cpu()
        ibits = torch.int32 if dtype == F32 else torch.int16
        assert torch.equal(got[:, cols:].contiguous().view(ibits), stored[:, cols:].contiguous().view(ibits)), what + ": pad columns written"
        assert torch.isfinite(got[:, :cols].float()).all(), what
        check(got[:, :cols], ref, dtype, what)
        if dtype == F32:
            off = fig(what + " |row sum - 1|", (got[:, :cols].double().sum(-1) - 1).abs().max().item(), 1e-5)
            assert off < 1e-5, (what, off)

    rows = torch.randn(6, cols, generator=g) * 30.0          # N(0, 30^2) at scale 0.3: logits of sigma 9
    rows[3] = 17.25                                           # a constant row: exactly uniform
    rows[4, -1] = rows[4].abs().max() + 40.0                  # the maximum in the last column
    run(rows, 0.3, f"softmax_rows {cols}")
    wide = (torch.rand(3, cols, generator=g) * 2 - 1) * 1e4   # a spread of +-1e4 at scale 1: finite, underflow to exact zeros allowed
    wide[1] = torch.linspace(-1e4, 1e4, cols)
    wide[2, 0] = 1e4
    run(wide, 1.0, f"softmax_rows {cols} wide")
