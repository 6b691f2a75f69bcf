"""The two kernels of unblur.hip - the 4 x 4 / stride 2 transposed conv and the GroupNorm + residual + SiLU tail - and the fp32 flash
attention at the face unblur network's shapes.

Criteria.  Exact transposed conv: integer operands whose partial sums stay below 2^24 make every product and sum exact in the hi / lo
plane format and in fp32, so the result must equal F.conv_transpose2d bit for bit.  Everything else is held to a float64 truth with
the error of an arm made of the kernels that existed before (tests/_unblur_cases.py `composed_*`, the unfused fp32 attention) as the
yardstick, measured in the same test on the same operands: the new route gets twice that, for a different summation order."""
import pytest
import torch
import torch.nn.functional as F

from tests import _unblur_cases as UC

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL = 776.0  # exact in the half types


def _cl(x):
    return x.to(DEV).contiguous(memory_format=torch.channels_last)


def _rel(got, truth):
    return UC.rel_l2(got, truth)


def _ints(name, shape, lo, hi):
    return torch.round(UC.synth(name, shape, 2.0)).clamp(lo, hi)


# ------------------------------------------------------------------------------------------------------------------- transposed conv
@pytest.mark.parametrize("batch", [2, 1])
@pytest.mark.parametrize("name,cin,cout,hw,act", UC.CONVT_CASES, ids=[c[0] for c in UC.CONVT_CASES])
def test_conv_transpose_exact(name, cin, cout, hw, act, batch):
    from cremage_amd import ops
    x = _ints(name + ".xi", (batch, cin) + hw, -4, 4)
    w = _ints(name + ".wi", (cin, cout, 4, 4), -3, 3)
    b = _ints(name + ".bi", (cout,), -8, 8) if act else None
    # every partial sum is an integer below 2^24: 4 Cin products of at most 12, plus the bias
    assert 4 * cin * 12 + 8 < 2 ** 24
    truth = F.conv_transpose2d(x.double(), w.double(), None if b is None else b.double(), stride=2, padding=1).float()
    assert torch.equal(UC.conv_transpose_parity(x, w, b), truth)
    hi, lo = ops.split_bf16(_cl(x))
    assert not bool(lo.any())
    wd = w.to(DEV)
    got = ops.conv_transpose2d(hi, lo, wd, None if b is None else b.to(DEV))
    route = ops.last_route()
    rows = batch * hw[0] * hw[1]  # the planner's three tile heights: 32 rows up to 64 source pixels, 64 up to 512, 128 beyond
    assert route["kernel"] == "convt" and route["config"] == (1 if rows <= 64 else 2 if rows <= 512 else 4) and route["wnt"] in (1, 2, 4), route
    assert tuple(got.shape) == (batch, cout, 2 * hw[0], 2 * hw[1]) and got.dtype == torch.float32
    assert torch.equal(got.cpu(), truth), (name, float((got.cpu() - truth).abs().max()))
    if act:  # ConvTransposeAct: the same sums, then SiLU - torch's own SiLU of the exact sums on the same device
        got = ops.conv_transpose2d(hi, lo, wd, b.to(DEV), silu=True)
        want = F.silu(truth.to(DEV))
        n_diff = int((got != want).sum())
        print(f"[fig] {name} B={batch}: SiLU epilogue differs from F.silu in {n_diff} of {want.numel()} values, "
              f"max {float((got - want).abs().max()):.3e}")
        assert torch.equal(got, want)
    # packed once: the second call finds the parity image in the weight cache
    from cremage_amd.ops._base import _pack_cache
    from cremage_amd import _lib as L
    assert _pack_cache.get((wd,), (L.PACK_CONVT_UP2, True)) is not None


@pytest.mark.parametrize("batch", [2, 1])
@pytest.mark.parametrize("name,cin,cout,hw,act", UC.CONVT_CASES, ids=[c[0] for c in UC.CONVT_CASES])
def test_conv_transpose_random(name, cin, cout, hw, act, batch):
    from cremage_amd import ops
    from cremage_amd.synth import synth_tensor
    x = UC.synth(name + ".x", (batch, cin) + hw)
    w = synth_tensor("unblur_ops." + name + ".weight", (cin, cout, 4, 4), UC.SEED)
    b = synth_tensor("unblur_ops." + name + ".bias", (cout,), UC.SEED) if act else None
    truth = F.conv_transpose2d(x.double(), w.double(), None if b is None else b.double(), stride=2, padding=1)
    if act:
        truth = F.silu(truth)
    xd, wd, bd = _cl(x), w.to(DEV), (None if b is None else b.to(DEV))
    w3, b3 = UC.composed_convt_weight(wd, bd)
    e_c = _rel(UC.composed_conv_transpose(xd, w3, b3, silu=act), truth)
    hi, lo = ops.split_bf16(xd)
    e_n = _rel(ops.conv_transpose2d(hi, lo, wd, bd, silu=act), truth)
    print(f"[fig] {name} B={batch}: new route {e_n:.3e} composed {e_c:.3e} bound {2 * e_c:.3e}")
    assert e_n <= 2 * e_c, (name, e_n, e_c)


def test_conv_transpose_refuses():
    from cremage_amd import ops
    from cremage_amd._lib import CrgError
    hi = torch.zeros((1, 16, 2, 2), dtype=ops.HALF, device=DEV)
    with pytest.raises(CrgError):
        ops.conv_transpose2d(hi, hi, torch.zeros((16, 8, 3, 3), device=DEV))  # not a 4 x 4 kernel
    with pytest.raises(CrgError):
        ops.conv_transpose2d(hi, hi, torch.zeros((16, 8, 4, 4), device=DEV).half())  # half-precision parameters
    with pytest.raises(CrgError):
        ops.conv_transpose2d(hi.float(), hi.float(), torch.zeros((16, 8, 4, 4), device=DEV))  # the fp32 tensor instead of planes


# ---------------------------------------------------------------------------------------------------------- GroupNorm + residual + SiLU
def _gn_truth(x, w, b, groups, skip, silu):
    y = F.group_norm(x.double(), groups, w.double(), b.double(), 1e-5)
    if skip is not None:
        y = y + skip.double()
    return F.silu(y) if silu else y


def _wide(n, c, h, w, dtype):
    buf = torch.full((n, h, w, c + 16), SENTINEL, dtype=dtype, device=DEV).permute(0, 3, 1, 2)
    return buf, buf[:, 8:8 + c]


def _rest_untouched(buf, c):
    return bool((buf[:, :8] == SENTINEL).all()) and bool((buf[:, 8 + c:] == SENTINEL).all())


@pytest.mark.parametrize("hw", UC.GN_HW, ids=[f"{h}x{w}" for h, w in UC.GN_HW])
@pytest.mark.parametrize("c,groups", UC.GN_CASES, ids=[f"c{c}_g{g}" for c, g in UC.GN_CASES])
def test_group_norm_add_act(c, groups, hw):
    from cremage_amd import ops
    from cremage_amd.synth import synth_tensor
    n, (h, w) = 2, hw
    tag = f"gn_{c}_{groups}_{h}x{w}"
    x = UC.synth(tag + ".x", (n, c, h, w), 1.5) + 0.25
    sk = UC.synth(tag + ".skip", (n, c, h, w))
    gw, gb = synth_tensor(tag + ".weight", (c,), UC.SEED), synth_tensor(tag + ".bias", (c,), UC.SEED)
    xd, skd, gwd, gbd = _cl(x), _cl(sk), gw.to(DEV), gb.to(DEV)
    for skip in (None, sk):
        for silu in (True, False):
            what = f"{tag} skip={skip is not None} silu={silu}"
            truth = _gn_truth(x, gw, gb, groups, skip, silu)
            s_d = None if skip is None else skd
            e_c = _rel(UC.composed_gn_add_act(xd, gwd, gbd, groups, 1e-5, s_d, silu)[0], truth)
            y, (hi, lo) = ops.group_norm_add_act(xd, gwd, gbd, groups, 1e-5, skip=s_d, silu=silu, planes=True)
            e_n = _rel(y, truth)
            print(f"[fig] {what}: kernel {e_n:.3e} composed {e_c:.3e} bound {2 * e_c:.3e}")
            assert e_n <= 2 * e_c, (what, e_n, e_c)
            shi, slo = ops.split_bf16(y)
            assert torch.equal(hi, shi) and torch.equal(lo, slo), what
            # the same call into column slices of wider buffers (offset 8 in rows of C + 16), the skip a slice as well
            ybuf, ydst = _wide(n, c, h, w, torch.float32)
            hbuf, hdst = _wide(n, c, h, w, ops.HALF)
            lbuf, ldst = _wide(n, c, h, w, ops.HALF)
            if s_d is not None:
                sbuf, sview = _wide(n, c, h, w, torch.float32)
                sview.copy_(skd)
                s_d = sview
            y2, (hi2, lo2) = ops.group_norm_add_act(xd, gwd, gbd, groups, 1e-5, skip=s_d, silu=silu, out=ydst, planes=(hdst, ldst))
            assert y2.data_ptr() == ydst.data_ptr() and hi2.data_ptr() == hdst.data_ptr()
            assert torch.equal(ydst, y) and torch.equal(hdst, hi) and torch.equal(ldst, lo), what
            assert _rest_untouched(ybuf, c) and _rest_untouched(hbuf, c) and _rest_untouched(lbuf, c), what
            # planes alone
            none, (hi3, lo3) = ops.group_norm_add_act(xd, gwd, gbd, groups, 1e-5, skip=s_d, silu=silu, planes=True, fp32=False)
            assert none is None and torch.equal(hi3, hi) and torch.equal(lo3, lo), what


@pytest.mark.parametrize("c,groups", [(64, 32), (112, 28)], ids=["c64_g32", "c112_g28"])
def test_group_norm_add_act_side_channel(c, groups):
    """x comes out of the fp32-class conv with its GroupNorm statistics side channel (32 x 32: the smallest image that has one)"""
    from cremage_amd import ops
    from cremage_amd.synth import synth_tensor
    n, h, w = 2, 32, 32
    tag = f"gn_side_{c}"
    x0 = UC.synth(tag + ".x0", (n, 64, h, w))
    wt = synth_tensor(tag + ".conv.weight", (c, 64, 3, 3), UC.SEED)
    gw, gb = synth_tensor(tag + ".weight", (c,), UC.SEED).to(DEV), synth_tensor(tag + ".bias", (c,), UC.SEED).to(DEV)
    sk = _cl(UC.synth(tag + ".skip", (n, c, h, w)))
    hi, lo = ops.split_bf16(_cl(x0))
    x = ops.conv2d(hi, wt.to(DEV), None, padding=1, x_lo=lo, gn_stats=True)
    assert ops._gn_stats_of(x, h * w) is not None, "the conv handed over no statistics"
    y, planes = ops.group_norm_add_act(x, gw, gb, groups, 1e-5, skip=sk, silu=True, planes=True)
    plain = x.clone(memory_format=torch.preserve_format)  # the same values without the side channel
    assert ops._gn_stats_of(plain, h * w) is None
    y_own, _ = ops.group_norm_add_act(plain, gw, gb, groups, 1e-5, skip=sk, silu=True)
    truth = _gn_truth(x.cpu(), gw.cpu(), gb.cpu(), groups, sk.cpu(), True)
    e_c = _rel(UC.composed_gn_add_act(plain, gw, gb, groups, 1e-5, sk, True)[0], truth)
    e_s, e_o = _rel(y, truth), _rel(y_own, truth)
    print(f"[fig] {tag}: with the side channel {e_s:.3e} own statistics {e_o:.3e} composed {e_c:.3e} bound {2 * e_c:.3e}")
    assert e_s <= 2 * e_c and e_o <= 2 * e_c
    shi, slo = ops.split_bf16(y)
    assert torch.equal(planes[0], shi) and torch.equal(planes[1], slo)


def test_group_norm_add_act_refuses():
    from cremage_amd import ops
    from cremage_amd._lib import CrgError
    x = torch.zeros((1, 16, 2, 2), device=DEV).contiguous(memory_format=torch.channels_last)
    g = torch.ones(16, device=DEV)
    with pytest.raises(CrgError):
        ops.group_norm_add_act(x, g, g, 3, 1e-5)  # groups do not divide C
    with pytest.raises(CrgError):
        ops.group_norm_add_act(x.half(), g, g, 4, 1e-5)  # fp32 class only
    with pytest.raises(CrgError):
        ops.group_norm_add_act(x, g, g, 4, 1e-5, fp32=False)  # nothing to write
    buf = torch.zeros((1, 2, 2, 32), device=DEV).permute(0, 3, 1, 2)
    with pytest.raises(CrgError):
        ops.group_norm_add_act(x, g, g, 4, 1e-5, out=buf[:, 2:18])  # rows not 16-byte aligned


# ---------------------------------------------------------------------------------------------------------------------- attention
@pytest.mark.parametrize("tokens,dh", UC.ATTN_CASES, ids=[f"t{t}_d{d}" for t, d in UC.ATTN_CASES])
def test_attention_at_model_shapes(tokens, dh):
    from cremage_amd import ops
    b, heads = 2, 8
    c = heads * dh
    tag = f"attn_{tokens}_{dh}"
    q, k, v = (UC.synth(f"{tag}.{s}", (b, tokens, c)) for s in "qkv")

    def truth():
        sp = lambda t: t.double().reshape(b, tokens, heads, dh).transpose(1, 2)  # noqa: E731
        a = torch.softmax(sp(q) @ sp(k).transpose(-1, -2) * dh ** -0.5, dim=-1)
        return (a @ sp(v)).transpose(1, 2).reshape(b, tokens, c)
    t64 = truth()
    ld = (tokens + 7) // 8 * 8
    vt = torch.zeros((b, c, ld), device=DEV)
    vt[:, :, :tokens] = v.to(DEV).transpose(1, 2)
    qd, kd = q.to(DEV), k.to(DEV)
    e_u = _rel(ops.attention(qd, kd, vt, heads, tokens, dh ** -0.5, flash=False), t64)
    e_f = _rel(ops.attention(qd, kd, vt, heads, tokens, dh ** -0.5, flash=True), t64)
    print(f"[fig] {tag}: flash {e_f:.3e} unfused {e_u:.3e} bound {2 * e_u:.3e}")
    assert e_f <= 2 * e_u, (tag, e_f, e_u)
