"""Bitwise GEMM / conv tests on exact operands, each on a route it asserts.

Operands are small integers (tests/_exact_cases.py: every fp32 partial sum is an exact integer below 2^24 in any order), so the fp64 CPU
result of F.linear / F.conv2d, converted ONCE to the output type, is the only right answer and the comparison is torch.equal.  The bias
puts half-type outputs where the type's spacing is 2 (384 for bfloat16, 3072 for fp16: computed from the type), so about half of them
are exact ties: a dropped or doubled product in one border column, truncation instead of round-to-nearest-even, a residual added behind
the rounding or a second rounding behind the split-K reduce all change bits here, where the Gaussian parity tests of
tests/test_hip_ops.py accept them (tests/test_exact_cpu.py demonstrates both halves of that sentence without a GPU).

Each case first asserts, from ops.last_route(), which kernel it ran; shapes reach a route by size alone (no environment knob is read or
set).  Generic over the process's half type like tests/test_hip_ops.py (CRG_HALF; tests/test_hip_ops_f16.py runs this file against the
fp16 build).

Out of scope because their arithmetic is not exact: SiLU and GEGLU epilogues, the LayerNorm epilogue (ln_stats), attention, the
application of GroupNorm.  The persistent ring GEMM (gemm_ring.hip) runs GEGLU only by default and stays on its tolerance test.  The
`launch_wnt<1, float, ...>` routes of the C ABI (fp32 input with the half-type product) are not reachable through cremage_amd.ops, which
hands fp32 activations to the fp32-class precision; they have no case here.

Statistics side channels (row_stats, gn_stats) are sums of integers and are compared with torch.equal against sums over the stored
output; such a case keeps the tie offset only where the sums of SQUARES of the stored output stay below 2^24 as well (bfloat16 with
32-row or half-tile partials).  With fp16 outputs (ties start at 2048) and with 256-row tile partials no offset meets that bound, so
those cases run on small integers: exact sums and order, no rounding.

MX conv (CRG_PREC_F16MX): values that are exact in the fp16 plane and in both e4m3 halves exist - a + k * 2^-13 with a in {-2, 0, 2},
|k| <= 3 against operands in {-1, 0, 1} (tests/_exact_cases.py::_mx_lo_values) - so each cross term has a case of its own.

Case -> route, as ops.last_route() reported it on MI355X (bfloat16 build; the fp16 build takes the same routes):
  case                          kernel    wnt cfg splits tail rowhalo lin pair up2 mx  reduce gn rows
  gemm_C_ragged                 glds        4   C      1    0       0   0    0   0  0  none         0
  gemm_C_k768                   glds        4   C      1    0       0   0    1   0  0  none         0
  gemm_D                        glds        5   D      1    0       0   0    1   0  0  none         0
  gemm_A_ktail                  glds        5   A      1    0       0   0    1   0  0  none         0
  gemm_splitk                   glds        5   A      3    0       0   0    0   0  0  plain        0
  gemm_tail_split               glds        5   A      1    4       0   0    1   0  0  plain        0
  gemm_ragged_n                 glds        4   C      1    0       0   0    1   0  0  none         0
  gemm_thin_n                   glds        1   C      1    0       0   0    1   0  0  none         0
  gemm_tokens_f32out            glds        4   C      1    0       0   0    0   0  0  none         0
  gemm_tokens                   glds        4   C      1    0       0   0    1   0  0  none         0
  gemm_vt                       glds        4   C      1    0       0   0    1   0  0  none         0
  gemm_row_stats_paired         glds        5   C      1    0       0   0    1   0  0  none         0
  gemm_row_stats_splitk         glds        5   A      3    0       0   0    0   0  0  rows         0
  gemm_gn_stats_paired          glds        4   C      1    0       0   0    1   0  0  none        32
  gemm_gn_stats_splitk          glds        5   A      3    0       0   0    0   0  0  stats       32
  rowres_k320                   (crg_ln_gemm: one kernel, no route record)
  conv_C_s1_fused               glds        4   C      1    0       0   0    1   0  0  none         0
  conv_C_stride2                glds        4   C      1    0       0   0    1   0  0  none         0
  conv_C_asym                   glds        4   C      1    0       0   0    1   0  0  none         0
  conv_C_upsample               glds        4   C      1    0       0   0    1   0  0  none         0
  conv_C_concat                 glds        4   C      1    0       0   0    1   0  0  none         0
  conv_C_concat_1x1             glds        4   C      1    0       0   0    1   0  0  none         0
  conv_C_odd                    glds        4   C      1    0       0   0    1   0  0  none         0
  conv_thin_out_wnt1            glds        1   C      1    0       0   0    1   0  0  none         0
  conv_rowhalo_unsplit_ragged   rowhalo     5   A      1    0       1   0    1   0  0  none         0
  conv_rowhalo_splitk_ragged    rowhalo     4   A      3    0       1   0    0   0  0  plain        0
  conv_halo_lin_w7              rowhalo     4   A      3    0       1   1    0   0  0  plain        0
  conv_halo_lin_w200            rowhalo     4   A      3    0       1   1    0   0  0  plain        0
  conv_pp_320                   conv_pp     5   A      1    0       2   0    1   0  0  none         0
  conv_pp_concat_128            conv_pp     4   A      1    0       2   0    1   0  0  none         0
  conv_pp_tile_stats            conv_pp     5   A      1    0       2   0    1   0  0  none       256
  conv_splitk_gn_reduce         rowhalo     4   A      3    0       1   1    0   0  0  gn           0
  conv_subpixel                 rowhalo     4   A      1    0       1   0    1   1  0  none         0
  conv_small_thin_in            (crg_conv_small: one kernel, no route record)
  conv_small_thin_out           (crg_conv_small: one kernel, no route record)
  x3_gemm_i                     gemm_reg    4   -      1    0       0   0    0   0  0  none         0
  planes_1x1_i                  planes      4   -      1    0       0   0    0   0  0  none         0
  planes_3x3_i                  planes      4   -      1    0       1   0    0   0  0  none         0
  planes_stride2_i              planes      4   -      1    0       0   0    0   0  0  none         0
  planes_subpixel_i             planes      4   -      1    0       1   0    0   1  0  none         0
  planes_splitk_i               planes      4   -      3    0       1   1    0   0  0  plain        0
  x3_gemm_ii                    gemm_reg    4   -      1    0       0   0    0   0  0  none         0
  planes_1x1_ii                 planes      4   -      1    0       0   0    0   0  0  none         0
  planes_3x3_ii                 planes      4   -      1    0       1   0    0   0  0  none         0
  planes_stride2_ii             planes      4   -      1    0       0   0    0   0  0  none         0
  planes_subpixel_ii            planes      4   -      1    0       1   0    0   1  0  none         0
  planes_splitk_ii              planes      4   -      3    0       1   1    0   0  0  plain        0
  x3_gemm_iii                   gemm_reg    4   -      1    0       0   0    0   0  0  none         0
  planes_1x1_iii                planes      4   -      1    0       0   0    0   0  0  none         0
  planes_3x3_iii                planes      4   -      1    0       1   0    0   0  0  none         0
  planes_stride2_iii            planes      4   -      1    0       0   0    0   0  0  none         0
  planes_subpixel_iii           planes      4   -      1    0       1   0    0   1  0  none         0
  planes_splitk_iii             planes      4   -      3    0       1   1    0   0  0  plain        0
  mx_3x3_i                      planes      4   -      1    0       1   0    0   0  1  none         0
  mx_3x3_ii                     planes      4   -      1    0       1   0    0   0  1  none         0
  mx_3x3_iii                    planes      4   -      1    0       1   0    0   0  1  none         0
"""
import os

import pytest
import torch

from tests import _exact_cases as E

pytestmark = pytest.mark.gpu

HALF_F16 = os.environ.get("CRG_HALF", "bf16").lower() in ("f16", "fp16", "float16", "half")  # cremage_amd/_lib.py:13 (no GPU call here)
BF = torch.float16 if HALF_F16 else torch.bfloat16


def _dev():
    assert torch.cuda.is_available(), "gpu tests need a HIP device"
    return torch.device("cuda:0")


def _img(t, dtype):
    return t.to(dtype).to(_dev()).contiguous(memory_format=torch.channels_last)


def assert_route(case, ops):
    if case.route is None:
        print(f"[route] {case.id}: (entry point without a route record)")
        return
    r = ops.last_route()
    print(f"[route] {case.id}: " + " ".join(f"{k}={v}" for k, v in r.items()))
    got = {k: r[k] for k in case.route}
    assert got == case.route, (case.id, "the shape no longer reaches the route this case is about", r)


def assert_same(got, exp, what, coords="mn"):
    """torch.equal, and on failure the count and the first coordinates that differ"""
    got = got.detach().cpu()
    assert got.dtype == exp.dtype and got.shape == exp.shape, (what, got.dtype, exp.dtype, got.shape, exp.shape)
    if torch.equal(got, exp):
        return
    bad = (got != exp) | torch.isnan(got.float())
    idx = bad.nonzero()
    first = [(tuple(i.tolist()), got[tuple(i)].item(), exp[tuple(i)].item()) for i in idx[:8]]
    raise AssertionError(f"{what}: {idx.shape[0]} of {got.numel()} elements differ; first ({', '.join(coords)}) (got, expected): {first}")


def run_case(case, ops, half):
    """the library's output (and side channels) for one case, the route asserted on the way"""
    o, ref, exp = E.prepared(case, half)
    dev = _dev()
    act = half if case.io in ("half", "f32out") else torch.float32
    out = half if case.io == "half" else torch.float32
    f32 = lambda t: None if t is None else t.float().to(dev)
    extra = {}
    if case.kind in ("gemm", "rowres"):
        M, N, K = case.shape
        lead = case.tokens or (M,)
        x = o["x"].to(act).to(dev).reshape(*lead, K)
        res = None if o["res"] is None else o["res"].to(out).to(dev).reshape(*lead, N)
        if case.kind == "rowres":
            y = ops.ln_linear(x, None, None, 0.0, o["w"].to(half).to(dev), f32(o["bias"]), residual=res)
        else:
            kw = {}
            if case.io == "f32out":
                kw["out_dtype"] = torch.float32
            if case.vt is not None:
                kw["transposed_from"] = case.vt
                assert ops.linear_transposed_ok(x, o["w"].float().to(dev), case.vt)
            if case.stats == "row":
                kw["row_stats"] = True
            if case.stats == "gn":
                kw["gn_hw"] = M
            y = ops.linear(x, o["w"].float().to(dev), f32(o["bias"]), residual=res, **kw)
            assert_route(case, ops)
            if case.vt is not None:
                y, extra["vt"] = y
            if case.stats == "row":
                st = getattr(y, "_crg_ln", None)
                assert st is not None and st[1] == y._version, "no row statistics came back"
                extra["row_stats"] = st[0]
            if case.stats == "gn":
                st = getattr(y, "_crg_gn_pending", None)
                assert st is not None, "no GroupNorm statistics came back"
                extra["gn_stats"] = st
        return y, extra
    n, c1, c2, h, w_, co = case.shape
    kw = {k: v for k, v in case.conv.items() if k not in ("ks", "gn")}
    if case.conv.get("gn"):
        kw["gn"] = (torch.ones(co, device=dev), torch.zeros(co, device=dev), 32, 1e-5, True)
    wd, bd = o["w"].float().to(dev), f32(o["bias"])
    kw.update(cvec=f32(o["cvec"]), residual=None if o["res"] is None else _img(o["res"], out))
    if case.stats == "gn":
        kw["gn_stats"] = True
    if case.io == "planes":
        hi, lo = ops.split_bf16(_img(o["x"], torch.float32))
        assert torch.equal(hi.double().cpu() + lo.double().cpu(), o["x"]), "the two planes do not hold x exactly"
        if case.opset == "ii":
            assert lo.float().abs().max().item() > 0, "set (ii) is meant to have a non-zero lo plane"
        y = ops.conv2d(hi, wd, bd, x_lo=lo, **kw)
    elif case.io == "mx":
        x16, x8 = ops.split_mx(_img(o["x"], torch.float32))
        y = ops.conv2d(x16, wd, bd, x_mx=x8, **kw)
    else:
        y = ops.conv2d(_img(o["x"], act), wd, bd, x2=_img(o["x2"], act) if c2 else None, **kw)
    assert_route(case, ops)
    if case.conv.get("gn"):
        y = y[0]
    if case.stats == "gn":
        st = getattr(y, "_crg_gn", None)
        assert st is not None, "no GroupNorm statistics came back"
        extra["gn_stats"], extra["gn_rows"] = st[0], (st[3] if len(st) > 3 else 32)
    return y, extra


def check_stats(case, y_rows, extra):
    """row_stats / gn_stats against exact sums over the STORED output (integers: fp32 sums in any order are exact below 2^24)"""
    rows = y_rows.double()
    if "row_stats" in extra:
        st = extra["row_stats"].cpu()                       # [M][parts][2]
        blk = E.stat_block(case)
        parts = st.shape[1]
        used = (rows.shape[1] + blk - 1) // blk             # (the split-K reduce: one whole-row partial, the others zero)
        assert used <= parts
        r = torch.nn.functional.pad(rows, (0, parts * blk - rows.shape[1])).reshape(rows.shape[0], parts, blk)
        assert (r * r).sum(2).max().item() < E.LIMIT
        assert_same(st[..., 0], r.sum(2).float(), case.id + " row_stats sums", "m,part")
        assert_same(st[..., 1], (r * r).sum(2).float(), case.id + " row_stats sums of squares", "m,part")
    if "gn_stats" in extra:
        blk = extra.get("gn_rows", 32)
        assert blk == E.stat_block(case)
        b = rows.reshape(-1, blk, rows.shape[1])
        assert (b * b).sum(1).max().item() < E.LIMIT
        st = extra["gn_stats"].cpu()[:, :b.shape[0]]        # tile partials fill the first M / rows rows of each plane
        assert_same(st[0], b.sum(1).float(), case.id + " gn_stats sums", "block,c")
        assert_same(st[1], (b * b).sum(1).float(), case.id + " gn_stats sums of squares", "block,c")


@pytest.mark.parametrize("case", E.CASES, ids=[c.id for c in E.CASES])
def test_exact(case):
    from cremage_amd import ops
    o, ref, exp = E.prepared(case, BF)
    y, extra = run_case(case, ops, BF)
    if case.kind == "conv":
        assert_same(y.permute(0, 2, 3, 1), exp.permute(0, 2, 3, 1), case.id, "nyxc")
        y_rows = y.permute(0, 2, 3, 1).reshape(-1, y.shape[1]).cpu()
    elif case.vt is not None:
        B, T = case.tokens
        e = exp.reshape(B, T, -1)
        assert y.shape == (B, T, case.vt) and extra["vt"].shape == (B, e.shape[2] - case.vt, (T + 7) // 8 * 8) and T % 8 != 0
        assert_same(y, e[..., :case.vt].contiguous(), case.id + " q | k", "btn")
        assert_same(extra["vt"][:, :, :T], e[..., case.vt:].transpose(1, 2).contiguous(), case.id + " v^T", "bnt")
        assert (extra["vt"][:, :, T:] == 0).all(), "pad columns of the transposed range must be exactly 0"
        y_rows = None
    else:
        assert_same(y.reshape(exp.shape), exp, case.id, "mn")
        y_rows = y.reshape(exp.shape).cpu()
    if case.stats:
        check_stats(case, y_rows, extra)


def test_route_record_is_cleared_by_a_failed_call():
    """crg_gemm clears the record on entry: a call that fails before it launches leaves kernel = none, not the previous call's route"""
    from cremage_amd import _lib, ops
    dev = _dev()
    ops.linear(torch.zeros(16, 64, dtype=BF, device=dev), torch.zeros(32, 64, device=dev))
    assert ops.last_route()["kernel"] == "glds"
    with pytest.raises(_lib.CrgError):
        ops.linear(torch.zeros(16, 12, dtype=BF, device=dev), torch.zeros(32, 12, dtype=BF, device=dev))  # K % 8 != 0: refused inside crg_gemm
    r = ops.last_route()
    assert r["kernel"] == "none" and r["reduce"] == "none" and all(v == 0 for k, v in r.items() if k not in ("kernel", "reduce")), r
