"""Batch-invariant mode (cremage_amd.set_batch_invariant) on a real MI355X: under the mode the bits the library
computes for one sample do not depend on the batch the sample sits in.

The check is the same for every case: ONE sample's inputs are fixed, the other samples of a batch are different random data; the
sample is run alone (B = 1) and at EVERY position of batches of 2, 3, 8 and 16 samples (3 and 9 where 16 would be large), and its
slice of every output - the statistics side channels and the transposed V range included - is `torch.equal` to the B = 1 result.
For crg_gemm / crg_conv2d the route record (ops.last_route()) is equal across B as well.  One case per family is repeated with
tune_samples = 1 (the small UNets and txt2img included: there every GEMM and conv takes the routes of one sample).

Still correct: every op case is also held against the result of the same call with the mode OFF, at the bound tests/test_hip_ops.py
puts on that op against its fp32 reference (`check`: rel-L2 6e-3 and max-abs 2^-6 * max|ref| + 1e-3 for the half type, times the
half type's HS; 5e-5 / 1e-4 * max|ref| + 1e-5 for the fp32 class; attention: rel-L2 1e-2 * HS, 5e-5 fp32), and the small models
against the committed goldens at the bounds of tests/test_hip_models.py (TOL_NET, TOL_SDXL_BF16).

The half type is the process's (CRG_HALF): tests/test_batch_invariant_f16.py runs this file against libcrg_hip_f16.so.
Every test here fails without the feature: the switch does not exist.
"""
import contextlib
import os

import pytest
import torch

from tests.conftest import load_golden, rel_l2

pytestmark = pytest.mark.gpu

HALF_F16 = os.environ.get("CRG_HALF", "bf16").lower() in ("f16", "fp16", "float16", "half")  # cremage_amd/_lib.py (no GPU call here)
BF = torch.float16 if HALF_F16 else torch.bfloat16
HS = 2.0 ** -3 if HALF_F16 else 1.0
DEV = "cuda:0"
TOL_NET = {torch.float32: 5e-5, BF: 2.5e-2}  # tests/test_hip_models.py
TOL_SDXL_BF16 = 3.3e-2                        # tests/test_hip_models.py
BATCHES = (2, 3, 8, 16)
BATCHES_BIG = (3, 9)


@contextlib.contextmanager
def mode(tune=8):
    import cremage_amd
    cremage_amd.set_batch_invariant(tune)
    try:
        yield
    finally:
        cremage_amd.set_batch_invariant(None)


def rnd(shape, seed, dtype=torch.float32, scale=1.0, shift=0.0):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return (torch.randn(shape, device=DEV, generator=g) * scale + shift).to(dtype)


def img(shape, seed, dtype, scale=1.0, shift=0.0):
    """[B, C, H, W] channels-last image"""
    b, c, h, w = shape
    return rnd((b, h, w, c), seed, dtype, scale, shift).permute(0, 3, 1, 2)


def bound_ok(got, ref, dtype, what, attention=False, group_norm=False):
    """the bounds of tests/test_hip_ops.py (`check`, the attention tests' rel-L2, and for the fp32 group_norm its own tighter ones:
    rel-L2 1e-5 and max-abs 2e-5 of test_group_norm_golden, max-abs 1e-4 where the output is hi + lo planes, whose resolution is
    2^-17 relative - test_split_planes_path / test_conv_planes_gn_stats), here against the mode-off result"""
    got, ref = got.detach().float().cpu(), ref.detach().float().cpu()
    assert got.shape == ref.shape and torch.isfinite(got).all(), what
    rel = ((got - ref).norm() / ref.norm().clamp_min(1e-20)).item()
    mx, scale = (got - ref).abs().max().item(), ref.abs().max().item()
    print(f"[fig] {what} vs mode off: rel-L2 {rel:.3e} max-abs {mx:.3e} (scale {scale:.3e})")
    if attention:
        assert rel < (1e-2 * HS if dtype == BF else 5e-5), (what, rel)
    elif group_norm and dtype != BF:
        assert rel < 1e-5 and mx < (1e-4 if group_norm == "planes" else 2e-5), (what, rel, mx)
    elif dtype == BF:
        assert rel < 6e-3 * HS and mx < (scale * 2 ** -6 + 1e-3) * HS, (what, rel, mx, scale)
    else:
        assert rel < 5e-5 and mx < scale * 1e-4 + 1e-5, (what, rel, mx, scale)


def same(got, ref, what):
    if torch.equal(got, ref):
        return
    bad = (got != ref) | torch.isnan(got.float())
    raise AssertionError(f"{what}: {int(bad.sum())} of {got.numel()} elements differ from the B = 1 result")


def invariance(run, sample, filler, batches, what, dtype=None, tune=8, route=False, attention=False, pick=None, correct=None, group_norm=False):
    """run(inputs) -> tuple of outputs with the sample dim first (and, with `route`, ops.last_route() behind them).  `sample`: tuple
    of one-sample inputs [1, ...]; filler(B): the same tuple for B other samples.  pick(outputs, p, B) -> the sample's slices
    (default: row p of every output).  dtype: also hold the outputs against the same call with the mode off, at the op's bound -
    the outputs of that dtype, or those `correct` lists (side channels change their granularity with the route and are checked by
    their consumers' outputs)."""
    from cremage_amd import ops
    pick = pick or (lambda outs, p, B: [o[p:p + 1] for o in outs])
    with mode(tune):
        ref = run(sample)
        r1 = ops.last_route() if route else None
        ref1 = [t.clone() for t in pick(ref, 0, 1)]
        for B in batches:
            base = filler(B)
            for p in range(B):
                batch = tuple(None if b is None else b.clone() for b in base)
                for t, s in zip(batch, sample):
                    if t is not None:
                        t[p] = s[0]
                outs = run(batch)
                if route:
                    rb = ops.last_route()
                    assert rb == r1, (what, B, p, "the route depends on the batch", r1, rb)
                for i, (o, r) in enumerate(zip(pick(outs, p, B), ref1)):
                    same(o, r, f"{what}: output {i}, position {p} of a batch of {B} (tune_samples {tune})")
    if route:
        print(f"[route] {what} (tune_samples {tune}): " + " ".join(f"{k}={v}" for k, v in r1.items()))
    if dtype is not None:  # still correct: the same call with the mode off, at the op's bound
        off = run(sample)
        for i, (o, r) in enumerate(zip(pick(off, 0, 1), ref1)):
            if (i in correct) if correct is not None else (o.dtype == dtype):
                bound_ok(r, o, dtype, f"{what} output {i}", attention, group_norm)
    return ref1


# ------------------------------------------------------------------------------------------ linear
def _gn_rows(stats, B, rows=32):
    """[2][M / 32][C] statistics planes -> [B][2][partials per sample][C] (tile partials fill the first M / rows rows of a plane)"""
    n = stats.shape[1] * 32 // rows
    return stats[:, :n].reshape(2, B, n // B, stats.shape[2]).transpose(0, 1)


LINEAR_CASES = {
    # id: (T, K, N, kwargs, batches)        between B = 1 and B = 16 these cross the C / D / A bounds, the ring bound and the split-K bound
    "t256_k1280": (256, 1280, 1280, {}, BATCHES),
    "t1024_k640_residual": (1024, 640, 640, dict(residual=True), BATCHES),
    "t64_k1280": (64, 1280, 1280, {}, BATCHES),
    "t4096_k320_geglu": (4096, 320, 2560, dict(act="geglu"), (2, 3, 8)),
    # the persistent 256-row kernel below its tuning point: 8 samples make 1280 tiles (its route), one sample 160 - fewer than CUs
    "t1024_k640_geglu_ring_small_grid": (1024, 640, 5120, dict(act="geglu"), (2, 8)),
    "t256_k640_fp32_class": (256, 640, 640, dict(fp32=True), BATCHES),
    "t77_k768_context": (77, 768, 320, {}, BATCHES),  # rows per sample that are no multiple of a tile: tiles straddle samples
}


def _linear_case(cid, tune=8, batches=None):
    from cremage_amd import ops
    T, K, N, kw, bs = LINEAR_CASES[cid]
    kw = dict(kw)
    dt = torch.float32 if kw.pop("fp32", False) else BF
    res = kw.pop("residual", False)
    w, b = rnd((N, K), 11, scale=K ** -0.5), rnd((N,), 12)
    n_out = N // 2 if kw.get("act") == "geglu" else N

    def run(inp):
        return (ops.linear(inp[0], w, b, residual=inp[1], **kw),)
    sample = (rnd((1, T, K), 1, dt), rnd((1, T, n_out), 2, dt) if res else None)
    invariance(run, sample, lambda B: (rnd((B, T, K), 100 + B, dt), rnd((B, T, n_out), 200 + B, dt) if res else None),
               batches or bs, "linear " + cid, dt, tune=tune, route=True)


@pytest.mark.parametrize("cid", list(LINEAR_CASES))
def test_linear(cid):
    _linear_case(cid)


def test_linear_tune_samples_1():
    _linear_case("t256_k1280", tune=1)
    _linear_case("t4096_k320_geglu", tune=1, batches=(2, 3))


def test_linear_ring_route_is_kept_on_small_grids():
    """the case above is about the persistent kernel on fewer tiles than CUs: say so from the route record"""
    from cremage_amd import ops
    w = rnd((5120, 640), 11, scale=640 ** -0.5)
    with mode(8):
        ops.linear(rnd((1, 1024, 640), 1, BF), w, None, act="geglu")
        assert ops.last_route()["kernel"] == "gemm_ring", ops.last_route()
    with mode(1):
        ops.linear(rnd((1, 1024, 640), 1, BF), w, None, act="geglu")
        assert ops.last_route()["kernel"] == "glds", ops.last_route()


def test_linear_tail_split_is_off_under_the_mode():
    """[8, 8224, 1024] -> 160: 8 x 8224 = 65792 rows are 514 = 512 + 2 tiles of configuration A on the two-blocks-per-CU kernel, the
    GEMM of tests/_exact_cases.py's gemm_tail_split as tokens of 8 samples.  8 samples are the tuning point, so what the heuristics read
    under the mode IS this call, and only the mode's own switch keeps the last two tiles - rows of the LAST sample - from being cut
    along K: the route says tail_splits = 0 at every position, the last one included, and the bits are those of the sample alone."""
    import cremage_amd
    from cremage_amd import ops
    T, K, N = 8224, 1024, 160
    w, b = rnd((N, K), 13, scale=K ** -0.5), rnd((N,), 14)
    big = rnd((8, T, K), 108, BF)
    ops.linear(big, w, b)  # the premise (mode off), as gemm_tail_split pins it: this call is one the default rule cuts
    off = ops.last_route()
    assert off["kernel"] == "glds" and off["config"] == 1 and off["tail_splits"] > 0, off

    def run(inp):
        y = ops.linear(inp[0], w, b)
        if cremage_amd.batch_invariant():
            r = ops.last_route()
            assert r["kernel"] == "glds" and r["config"] == 1 and r["splits"] == 1 and r["tail_splits"] == 0, (inp[0].shape, r)
        return (y,)
    invariance(run, (rnd((1, T, K), 1, BF),), lambda B: (big,), (8,), "linear 514 tiles", BF, route=True)


def test_linear_row_stats_feed_ln_linear_auto():
    """(4096, 320, 320) with row_stats=True: the output, its LayerNorm row statistics and the consumer that folds them"""
    from cremage_amd import ops
    T, K = 4096, 320
    w, b = rnd((K, K), 21, scale=K ** -0.5), rnd((K,), 22)
    w2, b2 = rnd((3 * K, K), 23, scale=K ** -0.5), rnd((3 * K,), 24)

    class LN:
        weight, bias, eps = 1 + 0.1 * rnd((K,), 25), 0.1 * rnd((K,), 26), 1e-5

    def run(inp):
        y = ops.linear(inp[0], w, b, row_stats=True)
        st = getattr(y, "_crg_ln", None)
        assert st is not None and st[1] == y._version, "no row statistics came back"
        B = y.shape[0]
        z = ops.ln_linear_auto(y, LN, w2, b2)
        return y, st[0].reshape(B, T, -1), z
    invariance(run, (rnd((1, T, K), 3, BF),), lambda B: (rnd((B, T, K), 300 + B, BF),), (2, 3, 8), "linear + row_stats -> ln_linear_auto", BF)


def test_linear_transposed_range():
    from cremage_amd import ops
    T, K, C = 256, 640, 640
    w, b = rnd((3 * C, K), 31, scale=K ** -0.5), rnd((3 * C,), 32)

    def run(inp):
        assert ops.linear_transposed_ok(inp[0], w, 2 * C)
        qk, vt = ops.linear(inp[0], w, b, transposed_from=2 * C)
        return qk, vt
    invariance(run, (rnd((1, T, K), 4, BF),), lambda B: (rnd((B, T, K), 400 + B, BF),), BATCHES, "linear transposed_from", BF, route=True)


@pytest.mark.parametrize("dt", ["half", "fp32"])
def test_linear_transposed(dt):
    """ops.linear_transposed: the samples lie along the GEMM's batch dimension"""
    from cremage_amd import ops
    dtype = BF if dt == "half" else torch.float32
    T, K, N = 200, 512, 512
    w, b = rnd((N, K), 33, scale=K ** -0.5), rnd((N,), 34)
    invariance(lambda inp: (ops.linear_transposed(inp[0], w, b),), (rnd((1, T, K), 5, dtype),), lambda B: (rnd((B, T, K), 500 + B, dtype),),
               BATCHES, "linear_transposed " + dt, dtype, route=True)


def test_time_rows_are_samples():
    """2-D inputs (the hoisted time rows): every row is a sample"""
    from cremage_amd import ops
    w, b = rnd((1280, 320), 35, scale=320 ** -0.5), rnd((1280,), 36)
    with mode(8):
        one = ops.linear(rnd((1, 320), 6, torch.float32), w, b, act="silu")
        many = rnd((160, 320), 7, torch.float32)
        many[77] = rnd((1, 320), 6, torch.float32)[0]
        same(ops.linear(many, w, b, act="silu")[77:78], one, "row 77 of 160 time rows")


# ------------------------------------------------------------------------------------------ conv2d
CONV_CASES = {
    # id: (Cin, Cout, H, W, conv kwargs, extras, batches)
    "c640_16x16": (640, 640, 16, 16, {}, "", BATCHES),          # the K slices change with N on today's rules
    "c1280_8x8": (1280, 1280, 8, 8, {}, "", BATCHES),
    "c320_32x32": (320, 320, 32, 32, {}, "", BATCHES),
    "c320_64x64_tail": (320, 320, 64, 64, {}, "", (8, 9)),      # 9 x 64 tiles: the 576-tile tail-split case
    "c320_32x32_stride2": (320, 320, 32, 32, dict(stride=2), "", BATCHES),
    "c640_16x16_upsample": (640, 640, 16, 16, dict(upsample2x=True), "", BATCHES),
    "c640_16x16_subpixel": (640, 640, 16, 16, dict(upsample2x=True, subpixel=True), "", BATCHES),
    "c640+320_16x16_concat_cvec_residual": (640, 640, 16, 16, {}, "x2 cvec res", BATCHES),
}


@pytest.mark.parametrize("cid", list(CONV_CASES))
def test_conv2d(cid):
    from cremage_amd import ops
    cin, cout, H, W, kw, extras, bs = CONV_CASES[cid]
    c2 = 320 if "x2" in extras else 0
    w, b = rnd((cout, cin + c2, 3, 3), 41, scale=(9 * (cin + c2)) ** -0.5), rnd((cout,), 42)
    ho = H // 2 if kw.get("stride") == 2 else (2 * H if kw.get("upsample2x") else H)

    def make(B, seed):
        return (img((B, cin, H, W), seed, BF), img((B, c2, H, W), seed + 1, BF) if c2 else None,
                rnd((B, cout), seed + 2) if "cvec" in extras else None, img((B, cout, ho, ho), seed + 3, BF) if "res" in extras else None)

    def run(inp):
        return (ops.conv2d(inp[0], w, b, x2=inp[1], cvec=inp[2], residual=inp[3], **kw),)
    invariance(run, make(1, 1), lambda B: make(B, 100 * B), bs, "conv2d " + cid, BF, route=True)


def test_conv2d_tune_samples_1():
    from cremage_amd import ops
    w, b = rnd((640, 640, 3, 3), 41, scale=5760 ** -0.5), rnd((640,), 42)
    invariance(lambda inp: (ops.conv2d(inp[0], w, b),), (img((1, 640, 16, 16), 1, BF),), lambda B: (img((B, 640, 16, 16), 100 * B, BF),),
               BATCHES, "conv2d c640_16x16", BF, tune=1, route=True)


@pytest.mark.parametrize("hw,rows", [(32, 32), (64, 256)])
def test_conv2d_gn_stats_and_consumer(hw, rows):
    """gn_stats on, followed by the group_norm that consumes them: the 32-row partial route (32 x 32) and the 256-row one (64 x 64)"""
    import cremage_amd
    from cremage_amd import ops
    C = 320
    w, b = rnd((C, C, 3, 3), 43, scale=(9 * C) ** -0.5), rnd((C,), 44)
    gw, gb = 1 + 0.1 * rnd((C,), 45), 0.1 * rnd((C,), 46)

    def run(inp):
        y = ops.conv2d(inp[0], w, b, gn_stats=True)
        st = getattr(y, "_crg_gn", None)
        assert st is not None, "no GroupNorm statistics came back"
        if cremage_amd.batch_invariant():  # (the mode-off comparison call takes whatever route the size of the call gives it)
            assert (st[3] if len(st) > 3 else 32) == rows, st[3:]
        return y, _gn_rows(st[0], y.shape[0], rows), ops.group_norm(y, gw, gb, 32, 1e-5, silu=True)
    invariance(run, (img((1, C, hw, hw), 2, BF),), lambda B: (img((B, C, hw, hw), 200 * B, BF),), BATCHES if hw == 32 else BATCHES_BIG,
               f"conv2d gn_stats {hw}x{hw}", BF)


def test_conv2d_fused_gn():
    """the gn= form on a conv cut along K: the launch that sums the slices normalises as well"""
    from cremage_amd import ops
    C = 1280
    w, b = rnd((C, C, 3, 3), 47, scale=(9 * C) ** -0.5), rnd((C,), 48)
    gn = (1 + 0.1 * rnd((C,), 49), 0.1 * rnd((C,), 50), 32, 1e-5, True)
    invariance(lambda inp: ops.conv2d(inp[0], w, b, gn=gn), (img((1, C, 8, 8), 3, BF),), lambda B: (img((B, C, 8, 8), 300 * B, BF),), BATCHES,
               "conv2d gn=", BF, route=True)


def test_conv2d_fp32_class_planes_with_statistics():
    """128 -> 128 at 64 x 64 on pre-split planes, its statistics side channel and the GroupNorm that consumes it"""
    from cremage_amd import ops
    C = 128
    w, b = rnd((C, C, 3, 3), 51, scale=(9 * C) ** -0.5), rnd((C,), 52)
    gw, gb = 1 + 0.1 * rnd((C,), 53), 0.1 * rnd((C,), 54)

    def run(inp):
        hi, lo = ops.split_bf16(inp[0])
        y = ops.conv2d(hi, w, b, x_lo=lo, gn_stats=True)
        st = getattr(y, "_crg_gn", None)
        assert st is not None, "no GroupNorm statistics came back"
        nh, nl = ops.group_norm(y, gw, gb, 32, 1e-6, silu=True, split=True)
        return y, _gn_rows(st[0], y.shape[0]), nh, nl, nh.float() + nl.float()
    invariance(run, (img((1, C, 64, 64), 4, torch.float32),), lambda B: (img((B, C, 64, 64), 400 * B, torch.float32),), BATCHES_BIG,
               "conv2d fp32-class planes", torch.float32, correct=(0, 4))


# ------------------------------------------------------------------------------------------ group_norm
@pytest.mark.parametrize("C,hw,c2,dtype,split", [(320, 64, 0, "half", False), (1280, 8, 0, "half", False), (320, 32, 320, "half", False),
                                                (128, 32, 0, "fp32", True), (128, 32, 0, "fp32", False)])
def test_group_norm(C, hw, c2, dtype, split):
    """stand-alone GroupNorm: the chunk doubling reads N today (C = 320 at 64 x 64: 1 sample against 8)"""
    from cremage_amd import ops
    dt = BF if dtype == "half" else torch.float32
    gw, gb = 1 + 0.1 * rnd((C + c2,), 55), 0.1 * rnd((C + c2,), 56)

    def run(inp):
        out = ops.group_norm(inp[0], gw, gb, 32, 1e-5, silu=True, x2=inp[1], split=split)
        return (out[0], out[1], out[0].float() + out[1].float()) if split else (out,)

    def make(B, seed):
        return (img((B, C, hw, hw), seed, dt, 2.0, 3.0), img((B, c2, hw, hw), seed + 1, dt, 2.0, 3.0) if c2 else None)
    invariance(run, make(1, 5), lambda B: make(B, 500 * B), (2, 8) if hw == 64 else BATCHES, f"group_norm C={C}+{c2} {hw}x{hw} {dtype}", dt,
               correct=(2,) if split else None, group_norm="planes" if split else True)


def test_group_norm_tune_samples_1():
    from cremage_amd import ops
    gw, gb = 1 + 0.1 * rnd((320,), 55), 0.1 * rnd((320,), 56)
    invariance(lambda inp: (ops.group_norm(inp[0], gw, gb, 32, 1e-5),), (img((1, 320, 32, 32), 5, BF, 2.0, 3.0),),
               lambda B: (img((B, 320, 32, 32), 500 * B, BF, 2.0, 3.0),), BATCHES, "group_norm C=320 32x32", BF, tune=1, group_norm=True)


# ------------------------------------------------------------------------------------------ attention
def _vt(v):
    """[B, Nk, C] -> the V^T operand [B, C, roundup(Nk, 8)], pads zeroed"""
    B, Nk, C = v.shape
    out = torch.zeros((B, C, (Nk + 7) // 8 * 8), dtype=v.dtype, device=v.device)
    out[:, :, :Nk] = v.transpose(1, 2)
    return out


ATTN_CASES = {
    # id: (heads, d, Nq, Nk, dtype, kwargs, batches)
    "cross_4096x77_d40": (8, 40, 4096, 77, "half", {}, (2, 8)),       # the few-keys kernel from nqg * B * H >= 2048 on today's rule
    "self_1024_d80": (8, 80, 1024, 1024, "half", {}, (2, 3, 8)),
    "self_256_d160": (8, 160, 256, 256, "half", {}, BATCHES),
    "unfused_fp32_256x77_d40": (8, 40, 256, 77, "fp32", dict(flash=False), (2, 3, 8)),
    "flash_fp32_256x77_d40": (8, 40, 256, 77, "fp32", dict(flash=True), (2, 3, 8)),
}


def _attention_case(cid, tune=8):
    from cremage_amd import ops
    heads, d, Nq, Nk, dtype, kw, bs = ATTN_CASES[cid]
    dt = BF if dtype == "half" else torch.float32
    C = heads * d

    def make(B, seed):
        return rnd((B, Nq, C), seed, dt), rnd((B, Nk, C), seed + 1, dt), _vt(rnd((B, Nk, C), seed + 2, dt))
    invariance(lambda inp: (ops.attention(inp[0], inp[1], inp[2], heads, Nk, d ** -0.5, **kw),), make(1, 6), lambda B: make(B, 600 * B), bs,
               "attention " + cid, dt, tune=tune, attention=True)


@pytest.mark.parametrize("cid", list(ATTN_CASES))
def test_attention(cid):
    _attention_case(cid)


def test_attention_tune_samples_1():
    _attention_case("cross_4096x77_d40", tune=1)


def test_attention_rows_v():
    from cremage_amd import ops
    heads, d, T = 8, 80, 1024
    C = heads * d

    def run(inp):
        qkv = inp[0]  # column slices of one fused projection output
        return (ops.attention_rows_v(qkv[..., :C], qkv[..., C:2 * C], qkv[..., 2 * C:], heads, d ** -0.5),)
    invariance(run, (rnd((1, T, 3 * C), 7, BF),), lambda B: (rnd((B, T, 3 * C), 700 * B, BF),), (2, 3, 8), "attention_rows_v", BF, attention=True)


# ------------------------------------------------------------------------------------------ layer_norm, softmax_rows_
@pytest.mark.parametrize("dtype", ["half", "fp32"])
def test_layer_norm(dtype):
    """a handful of rows against many: 16 x 1024 rows cross the rows-per-wave bound of today's rule"""
    from cremage_amd import ops
    dt = BF if dtype == "half" else torch.float32
    g, b = 1 + 0.1 * rnd((320,), 61), 0.1 * rnd((320,), 62)
    invariance(lambda inp: (ops.layer_norm(inp[0], g, b),), (rnd((1, 1024, 320), 8, dt, 1.0, 0.5),), lambda B: (rnd((B, 1024, 320), 800 * B, dt, 1.0, 0.5),),
               BATCHES, "layer_norm " + dtype, dt)
    with mode(8):  # four rows alone
        few = rnd((1, 4, 320), 9, dt)
        many = rnd((16, 1024, 320), 10, dt)
        many[5, 100:104] = few[0]
        same(ops.layer_norm(many, g, b)[5, 100:104], ops.layer_norm(few, g, b)[0], "four rows among 16384")


def test_softmax_rows():
    from cremage_amd import ops
    invariance(lambda inp: (ops.softmax_rows_(inp[0].clone(), 77, 0.3),), (rnd((1, 64, 80), 11, torch.float32, 3.0),),
               lambda B: (rnd((B, 64, 80), 1100 * B, torch.float32, 3.0),), BATCHES, "softmax_rows_", torch.float32)


def test_layer_norm_and_softmax_rows_tune_samples_1():
    from cremage_amd import ops
    g, b = 1 + 0.1 * rnd((320,), 61), 0.1 * rnd((320,), 62)
    invariance(lambda inp: (ops.layer_norm(inp[0], g, b),), (rnd((1, 1024, 320), 8, BF, 1.0, 0.5),), lambda B: (rnd((B, 1024, 320), 800 * B, BF, 1.0, 0.5),),
               BATCHES, "layer_norm half", BF, tune=1)
    invariance(lambda inp: (ops.softmax_rows_(inp[0].clone(), 77, 0.3),), (rnd((1, 64, 80), 11, torch.float32, 3.0),),
               lambda B: (rnd((B, 64, 80), 1100 * B, torch.float32, 3.0),), BATCHES, "softmax_rows_", torch.float32, tune=1)


# ------------------------------------------------------------------------------------------ MX8 feed-forward (opt-in path)
def test_mx8_feed_forward_chain():
    """quant_mx8 -> linear_mx8 (GEGLU, MX8 out) -> linear_mx8 + residual: one kernel per problem class, one block per tile of rows"""
    from cremage_amd import ops
    T, K, F = 256, 640, 2560
    w1, b1 = rnd((2 * F, K), 71, scale=K ** -0.5), rnd((2 * F,), 72)
    w2, b2 = rnd((K, F), 73, scale=F ** -0.5), rnd((K,), 74)

    def run(inp):
        assert ops.ff_mx8_ok(inp[0], w1, w2)
        hq, he = ops.linear_mx8(*ops.quant_mx8(inp[0]), w1, b1, act="geglu", out="mx8")
        return (ops.linear_mx8(hq, he, w2, b2, residual=inp[0], out="half"),)
    invariance(run, (rnd((1, T, K), 12, BF),), lambda B: (rnd((B, T, K), 1200 * B, BF),), BATCHES, "MX8 feed-forward", BF)


# ------------------------------------------------------------------------------------------ models
def _model_invariance(m, make, images, what, cfg_mark=False, graphed=False, tune=8):
    """make(b, seed) -> (x [b, ...], kwargs of per-sample tensors [b, ...]); with cfg_mark the call is the CFG-doubled batch
    cat([x, x]) whose conditioning halves differ (kwargs come as [2 b, ...], unconditional half first)"""
    from cremage_amd import ops
    from cremage_amd.graphs import GraphedModule
    call = GraphedModule(m, scratch_bytes=64 << 20) if graphed else m

    def run(x, kw):
        if cfg_mark:
            x = ops.mark_cfg_dup(torch.cat([x, x]))
        with torch.no_grad():
            return call(x, **kw)

    def put(batch, b, p, sample):
        """write the fixed sample to position p of a batch of b images"""
        (bx, bkw), (sx, skw) = batch, sample
        bx[p] = sx[0]
        for k in bkw:
            if cfg_mark and k != "timesteps_half":
                bkw[k][p], bkw[k][b + p] = skw[k][0], skw[k][1]
            else:
                bkw[k][p] = skw[k][0]

    def expand(kw):
        kw = dict(kw)
        th = kw.pop("timesteps_half", None)
        if th is not None:
            kw["timesteps"] = torch.cat([th, th]) if cfg_mark else th
        return kw
    with mode(tune):
        sample = make(1, 1)
        ref = run(sample[0], expand(sample[1])).clone()
        for b in images:
            base = make(b, 10 * b)
            for p in range(b):
                batch = (base[0].clone(), {k: v.clone() for k, v in base[1].items()})
                put(batch, b, p, sample)
                out = run(batch[0], expand(batch[1]))
                same(out[p], ref[0], f"{what}: image {p} of {b} (tune_samples {tune})")
                if cfg_mark:
                    same(out[b + p], ref[1], f"{what}: image {p} of {b}, conditional half")
    return ref


def _unet_inputs(cfg, L, cfg_mark, sdxl=False):
    def make(b, seed):
        n = 2 * b if cfg_mark else b
        kw = dict(timesteps_half=torch.full((b,), 801.5, device=DEV) - rnd((b,), seed + 3).abs() * 50,
                  context=rnd((n, 77, cfg["context_dim"]), seed + 1))
        if sdxl:
            kw["y"] = rnd((n, cfg["adm_in_channels"]), seed + 2)
        return rnd((b, 4, L, L), seed), kw
    return make


@pytest.mark.parametrize("graphed", [False, True], ids=["eager", "graphed"])
@pytest.mark.parametrize("cfg_mark", [False, True], ids=["plain", "cfg"])
@pytest.mark.parametrize("name", ["unet_small_sd", "sgm_unet_small_sdxl"])
def test_unet_small(name, cfg_mark, graphed):
    """the small SD1.5 / SDXL UNet configurations of the golden generator at 32 x 32 latents: batch 1 against every position of
    batches of 3 and 5 images; and, still correct, the committed golden under the mode"""
    sdxl = name.startswith("sgm")
    if sdxl:
        from cremage_amd.sgm_hip.unet import UNetModel
    else:
        from cremage_amd.ldm_hip.unet import UNetModel
    from cremage_amd.synth import synth_fill_, synth_input
    meta, g = load_golden(name)
    cfg = meta["cfg"]
    m = synth_fill_(UNetModel(**cfg), meta["seed"], prefix=meta["prefix"]).to(BF).to(DEV).eval()
    _model_invariance(m, _unet_inputs(cfg, 32, cfg_mark, sdxl), (3, 5), name, cfg_mark, graphed)
    if not cfg_mark and not graphed:
        x = synth_input(name + ".x", (meta["B"], 4, meta["L"], meta["L"]), meta["seed"]).to(DEV)
        kw = dict(timesteps=g["t"].to(DEV), context=synth_input(name + ".ctx", (meta["B"], meta["m"], cfg["context_dim"]), meta["seed"]).to(DEV))
        if sdxl:
            kw["y"] = synth_input(name + ".y", (meta["B"], cfg["adm_in_channels"]), meta["seed"]).to(DEV)
        with mode(8), torch.no_grad():
            y = m(x, **kw)
        r = rel_l2(y.float().cpu(), g["y"])
        print(f"[fig] {name} under the mode vs golden: rel-L2 {r:.3e}")
        assert r < (TOL_SDXL_BF16 if sdxl else TOL_NET[BF]), r


@pytest.mark.parametrize("name", ["unet_small_sd", "sgm_unet_small_sdxl"])
def test_unet_small_tune_samples_1(name):
    """the worst-tuned point: every GEMM and conv of the UNet on the routes of ONE sample (small grids, deep K cuts), CFG-marked"""
    sdxl = name.startswith("sgm")
    if sdxl:
        from cremage_amd.sgm_hip.unet import UNetModel
    else:
        from cremage_amd.ldm_hip.unet import UNetModel
    from cremage_amd.synth import synth_fill_
    meta, _ = load_golden(name)
    m = synth_fill_(UNetModel(**meta["cfg"]), meta["seed"], prefix=meta["prefix"]).to(BF).to(DEV).eval()
    _model_invariance(m, _unet_inputs(meta["cfg"], 32, True, sdxl), (3, 5), name, cfg_mark=True, tune=1)


def test_controlnet_small():
    """the small ControlNet: its 13 control tensors and eps through ControlLDM.apply_model, batch 1 against batches of 3 and 5"""
    from cremage_amd.cldm_hip import ControlLDM, ControlledUnetModel, ControlNet
    from cremage_amd.ldm_hip.vae import AutoencoderKL
    from cremage_amd.synth import synth_fill_, synth_input
    meta, g = load_golden("controlnet_small_sd")
    cfg = meta["cfg"]
    cn = ControlNet(hint_channels=3, **{k: v for k, v in cfg.items() if k != "out_channels"})
    un = ControlledUnetModel(**cfg)
    synth_fill_(cn, meta["seed"], prefix=meta["cn_prefix"])
    synth_fill_(un, meta["seed"], prefix=meta["unet_prefix"])
    vae = AutoencoderKL(dict(double_z=True, z_channels=4, resolution=32, in_channels=3, out_ch=3, ch=32, ch_mult=[1, 2], num_res_blocks=1,
                             attn_resolutions=[], dropout=0.0), None, 4)
    ldm = ControlLDM(cn, "hint", False, un, vae).to(BF).to(DEV).eval()
    L = 32

    def run(x, hint, t, ctx):
        with torch.no_grad():
            control = ldm.control_model(x=x, hint=hint, timesteps=t, context=ctx)
            eps = ldm.apply_model(x, t, {"c_crossattn": [ctx], "c_concat": [hint]})
        return list(control) + [eps]

    def make(b, seed):
        return [rnd((b, 4, L, L), seed), (rnd((b, 3, 8 * L, 8 * L), seed + 1, scale=0.25) + 0.5).clamp(0, 1),
                torch.full((b,), 801.5, device=DEV) - rnd((b,), seed + 2).abs() * 50, rnd((b, 77, cfg["context_dim"]), seed + 3)]
    with mode(8):
        sample = make(1, 1)
        ref = [t.clone() for t in run(*sample)]
        assert len(ref) == meta["n_control"] + 1
        for b in (3, 5):
            base = make(b, 10 * b)
            for p in range(b):
                batch = [t.clone() for t in base]
                for t, s in zip(batch, sample):
                    t[p] = s[0]
                for i, (o, r) in enumerate(zip(run(*batch), ref)):
                    same(o[p:p + 1], r, f"controlnet output {i}: image {p} of {b}")
        # still correct: the committed golden (B = 2, 16 x 16 latents) under the mode, at tests/test_hip_models.py's bound
        B, Lg, seed = meta["B"], meta["L"], meta["seed"]
        x = synth_input("cnet.x", (B, 4, Lg, Lg), seed).to(DEV)
        hint = (synth_input("cnet.hint", (B, 3, 8 * Lg, 8 * Lg), seed, 0.5).clamp(-1, 1) * 0.5 + 0.5).to(DEV)
        ctx = synth_input("cnet.ctx", (B, 77, cfg["context_dim"]), seed).to(DEV)
        outs = run(x, hint, g["t"].to(DEV), ctx)
        for i, c in enumerate(outs[:-1]):
            assert rel_l2(c.float().cpu().contiguous(), g[f"control{i}"]) < TOL_NET[BF], i
        assert rel_l2(outs[-1].float().cpu(), g["eps"]) < TOL_NET[BF]


def test_vae_decode_and_encode():
    """fp32-class VAE: decode of a 16 x 16 latent and encode of its 32 x 32 image, batch 1 against batches of 3 and 5; the committed
    golden under the mode at the bounds of tests/test_hip_models.py::test_vae_tiny"""
    from cremage_amd.ldm_hip.vae import AutoencoderKL
    from cremage_amd.synth import synth_fill_
    meta, g = load_golden("vae_tiny")
    vae = synth_fill_(AutoencoderKL(meta["dd"], None, 4), meta["seed"], prefix=meta["prefix"]).to(DEV).eval()
    with mode(8), torch.no_grad():
        z1, i1 = rnd((1, 4, 16, 16), 1), rnd((1, 3, 32, 32), 2, scale=0.5).clamp(-1, 1)
        dec1, enc1 = vae.decode(z1).clone(), vae.encode(i1).parameters.clone()
        for b in (3, 5):
            zb, ib = rnd((b, 4, 16, 16), 10 * b), rnd((b, 3, 32, 32), 10 * b + 1, scale=0.5).clamp(-1, 1)
            for p in range(b):
                z, im = zb.clone(), ib.clone()
                z[p], im[p] = z1[0], i1[0]
                same(vae.decode(z)[p:p + 1], dec1, f"VAE decode: image {p} of {b}")
                same(vae.encode(im).parameters[p:p + 1], enc1, f"VAE encode: image {p} of {b}")
        from cremage_amd.synth import synth_input
        z = synth_input("vae_tiny.z", (2, 4, 8, 8), meta["seed"]).to(DEV)
        im = synth_input("vae_tiny.img", (2, 3, 16, 16), meta["seed"], 0.5).clamp(-1, 1).to(DEV)
        assert rel_l2(vae.decode(z).float().cpu(), g["dec"]) < TOL_NET[torch.float32]
        assert rel_l2(vae.encode(im).parameters.float().cpu(), g["moments"]) < TOL_NET[torch.float32]


# ------------------------------------------------------------------------------------------ end to end
def _small_ldm():
    from cremage_amd import pipeline as P
    meta, _ = load_golden("traj_euler_a")
    return P.build_synthetic_ldm(meta["unet"], meta["dd"], DEV, unet_dtype=BF, vae_dtype=torch.float32, seed=meta["seed"]), meta


def _gens(seed, indices):
    from cremage_amd.dist import image_seed
    return [torch.Generator(device=DEV).manual_seed(image_seed(seed, i)) for i in indices]


@pytest.mark.parametrize("sampler,tune", [("euler_a", 8), ("dpmpp_2m", 8), ("euler_a", 1)])
def test_txt2img_batch_of_three_equals_three_single_calls(sampler, tune):
    """3 steps, CFG, generators=[image_seed(seed, i)]: latents and images of a batch of 3 are those of three batch-1 calls - and of
    the same images sharded (2, 1) and (1, 1, 1) with dist.shard_range"""
    from cremage_amd import pipeline as P
    from cremage_amd.dist import shard_range
    ldm, meta = _small_ldm()
    L, seed = 32, 4321
    c, uc = rnd((3, 77, 96), 81), rnd((3, 77, 96), 82)

    def run(idx):
        idx = list(idx)
        return P.txt2img(ldm, c[idx], uc[idx], steps=3, sampler=sampler, cfg_scale=7.5, height=8 * L, width=8 * L, generators=_gens(seed, idx))
    with mode(tune):
        images, latents = run(range(3))
        for world in (1, 2, 3):  # shard sizes (3), (2, 1), (1, 1, 1)
            parts = [run(shard_range(3, rank, world)) for rank in range(world)]
            same(torch.cat([p[1] for p in parts]), latents, f"{sampler}: latents of {world} shards")
            same(torch.cat([p[0] for p in parts]), images, f"{sampler}: images of {world} shards")
    assert torch.isfinite(images).all() and 0 <= images.min() and images.max() <= 1 and images.std() > 1e-3


def test_ddim_img2img_batch_of_three_equals_three_single_calls():
    from cremage_amd import pipeline as P
    ldm, meta = _small_ldm()
    L = 16
    c, uc = rnd((3, 77, 96), 83), rnd((3, 77, 96), 84)
    init = rnd((3, 3, 2 * L, 2 * L), 85, scale=0.5).clamp(-1, 1)  # (this VAE has one downsampling level)
    en, fn = rnd((3, 4, L, L), 86), rnd((3, 4, L, L), 87)

    def run(idx):
        return P.img2img(ldm, init[idx], c[idx], uc[idx], steps=20, strength=0.15, cfg_scale=7.5, enc_noise=en[idx], fwd_noise=fn[idx])
    with mode(8):
        images, latents = run([0, 1, 2])
        for i in range(3):
            im, la = run([i])
            same(la, latents[i:i + 1], f"DDIM img2img latents, image {i}")
            same(im, images[i:i + 1], f"DDIM img2img image {i}")


# ------------------------------------------------------------------------------------------ the switch itself
def test_mode_off_routes_are_untouched():
    """after set_batch_invariant(None) the size-dependent route cases of tests/_exact_cases.py report the routes they report today
    (tests/test_exact_gpu.py::run_case asserts the route and the exact result)"""
    import cremage_amd
    from cremage_amd import ops
    from tests import _exact_cases as E
    from tests.test_exact_gpu import run_case
    cremage_amd.set_batch_invariant(8)
    assert cremage_amd.batch_invariant() == 8
    cremage_amd.set_batch_invariant(None)
    assert cremage_amd.batch_invariant() == 0
    for cid in ("gemm_tail_split", "gemm_D", "conv_pp_320"):
        run_case(E.BY_ID[cid], ops, BF)


def test_mode_is_set_on_live_and_later_contexts():
    import cremage_amd
    from cremage_amd import _lib
    h0 = _lib.ctx(0)
    with mode(5):
        assert _lib.load().crg_ctx_get_invariant(h0) == 5
        prev = _lib.set_lane(7)  # a context created under the mode
        try:
            assert _lib.load().crg_ctx_get_invariant(_lib.ctx(0)) == 5
        finally:
            _lib.set_lane(prev)
    assert _lib.load().crg_ctx_get_invariant(h0) == 0
    assert _lib.load().crg_ctx_set_invariant(h0, -1) != 0  # negative: refused, the state stays
    assert _lib.load().crg_ctx_get_invariant(h0) == 0 and cremage_amd.batch_invariant() == 0


def test_rows_per_sample_must_divide_the_rows():
    """under the mode a GEMM whose rows are no whole number of samples is an error, not a guess"""
    from cremage_amd import _lib, ops
    x, w = rnd((100, 64), 93, BF), rnd((64, 64), 94, BF)
    y = torch.empty((100, 64), dtype=BF, device=DEV)
    kw = dict(a=x.data_ptr(), lda=64, w=w.data_ptr(), ldw=64, y=y.data_ptr(), ldy=64, M=100, N=64, K=64, batch=1, a_dtype=_lib.BF16, y_dtype=_lib.BF16,
              prec=_lib.PREC_BF16, rows_per_sample=30)
    ops._gemm(_lib.ctx(0), **kw)  # mode off: the field is ignored
    with mode(8):
        with pytest.raises(_lib.CrgError, match="rows_per_sample"):
            ops._gemm(_lib.ctx(0), **kw)
        ops._gemm(_lib.ctx(0), **dict(kw, rows_per_sample=0))  # 0 means 1
