"""The conv behind a nearest-2x upsample in its sub-pixel form (crg_conv_args.upsample2x = 2): four 2x2 convs on the source grid, one per
output parity, with the 3x3 taps that read the same source pixel summed at pack time (CRG_PACK_CONV_UP2) - 4 / 9 of the multiplies.

Reference: the fp64 conv of the upsampled, storage-rounded input (what tests/test_hip_ops.py::conv_ref computes, in fp64); bounds:
check()'s own.  The summed weights are rounded once more than the plain ones: measured on MI355X, rel-L2 2.3e-3 in bf16 (gather form
1.7e-3; bound 6e-3), 2.8e-4 in fp16 (7.5e-4), 3.2e-6 on fp32-class planes (5e-5).

Each shape isolates one thing that can go wrong (see the ids); two shapes the predicate refuses keep the gather form and must still be
right.  What a launch leaves visible is asserted through ops.profile: the kernel slot (160- / 128-wide tiles, split planes) and whether
the split-K reduce kernel ran.  128- against 256-row tiles is not visible from outside the library: the two `tiles_of_256_rows` shapes give
exactly 256 blocks of 256 rows (one full round of the 256 CUs, the launch rule asks for 85 %), the others fewer than 85 % of a round.
16-bit operands take the form only with subpixel=True: by default (the UNet's Upsample layer) they keep the gather form's bits, because
weights rounded once more would move the sampler trajectory.  The last test runs this file against the fp16 library in a child process."""
import ctypes as C
import os
import re
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

from test_hip_ops import BF, HS, _dev, check, fig, nhwc, q, rnd

pytestmark = pytest.mark.gpu

# (dtype, N, C, H, W, Cout, statistics side channel checked as well, kernel slot of the conv, split-K reduce launches expected)
CASES = {
    "rows_r8_one_chunk": (BF, 2, 64, 16, 16, 64, True, "conv_w4", False),   # rows geometry, R = 8, one chunk, all four image borders in one tile set
    "two_chunks_partial_ntile": (BF, 1, 128, 32, 32, 96, False, "conv_w4", False),  # two chunks, partial last n-tile (H W a multiple of 256)
    "splitk_reduce_remap": (BF, 1, 1280, 16, 16, 160, True, "conv_w5", True),  # 80 k-tiles on 8 tiles: split-K, the reduce kernel's row remap
    "segments": (BF, 1, 64, 2, 256, 64, False, "conv_w4", False),           # segment geometry, W > tile
    "planes_rows": (torch.float32, 1, 128, 64, 64, 128, True, "conv_x3", None),  # fp32-class planes (ops.split_bf16)
    "planes_segments": (torch.float32, 1, 64, 2, 256, 64, False, "conv_x3", None),
    # beyond the issue's list: 32 x 8 = 256 tiles of 256 rows, the 8-wave arm (8 x 1280 x 16 x 16 sized launches) - paired epilogue on
    # 160-wide tiles, and the plain one (Cout no multiple of 8) on 128-wide tiles
    "tiles_of_256_rows": (BF, 8, 64, 16, 16, 1280, True, "conv_w5", False),
    "tiles_of_256_rows_plain_epilogue": (BF, 8, 64, 16, 16, 1020, False, "conv_w4", False),
}


def ref64(x, w, b, dtype):
    xx = F.interpolate(q(x, dtype).double(), scale_factor=2, mode="nearest")
    return F.conv2d(xx, (q(w, BF) if dtype == BF else w).double(), b.double(), padding=1)


def inputs(N, Cin, H, W, Co, seed):
    return rnd(N, Cin, H, W, seed=seed), rnd(Co, Cin, 3, 3, seed=seed + 1, scale=(9 * Cin) ** -0.5), rnd(Co, seed=seed + 2)


def run(x, w, b, dtype, gn_stats=False):
    from cremage_amd import ops
    dev = _dev()
    if dtype == BF:
        xs, lo = nhwc(x, BF), None
    else:
        xs, lo = ops.split_bf16(nhwc(x, torch.float32))
    ok = ops.upsample_subpixel_ok(xs, w.to(dev), lo)
    with ops.profile() as prof:
        y = ops.conv2d(xs, w.to(dev), b.to(dev), upsample2x=True, x_lo=lo, gn_stats=gn_stats, subpixel=True)
    return ok, y, {k: v["launches"] for k, v in prof.kernels.items() if v["launches"]}


@pytest.mark.parametrize("case", list(CASES))
def test_subpixel_conv(case):
    from cremage_amd import ops
    dtype, N, Cin, H, W, Co, stats, slot, reduce = CASES[case]
    x, w, b = inputs(N, Cin, H, W, Co, 700)
    ok, y, launches = run(x, w, b, dtype, gn_stats=stats)
    assert ok, "the predicate refused a shape the sub-pixel form is built for"
    assert launches.get(slot) == 1, launches
    if reduce is not None:
        assert ("splitk_reduce" in launches) == reduce, launches
    assert y.dtype == dtype and tuple(y.shape) == (N, Co, 2 * H, 2 * W)
    check(y, ref64(x, w, b, dtype), dtype, f"sub-pixel upsample conv {case}")
    if not stats:
        return
    # the GroupNorm statistics side channel (written in the kernel's virtual row order, per-sample contiguous): group_norm() on the
    # tensor that carries it against group_norm() on a clone, which computes its own - the bounds of test_gn_stats_side_channel (half
    # type) and test_conv_planes_gn_stats (planes) in tests/test_hip_ops.py
    dev = _dev()
    assert getattr(y, "_crg_gn", None) is not None, "the conv did not hand over statistics"
    gam, bet = (1 + 0.1 * rnd(Co, seed=720)).to(dev), (0.1 * rnd(Co, seed=721)).to(dev)
    if dtype == BF:
        fast = ops.group_norm(y, gam, bet, 32, 1e-5, silu=True)
        plain = ops.group_norm(y.clone(memory_format=torch.preserve_format), gam, bet, 32, 1e-5, silu=True)
        refn = F.silu(F.group_norm(y.float().cpu(), 32, gam.cpu(), bet.cpu(), 1e-5))
        check(fast, refn, BF, case + " gn(pre)")
        d = fig(case + " gn(pre) vs gn(own statistics)", (fast.float() - plain.float()).abs().max().item(), 2 ** -6 * HS * refn.abs().max().item())
        assert d <= 2 ** -6 * HS * refn.abs().max().item()
    else:
        nh, nl = ops.group_norm(y, gam, bet, 32, 1e-6, silu=True, split=True)
        rh, rl = ops.group_norm(y.clone(memory_format=torch.preserve_format), gam, bet, 32, 1e-6, silu=True, split=True)
        refn = F.silu(F.group_norm(y.double().cpu(), 32, gam.double().cpu(), bet.double().cpu(), 1e-6))
        e_pre = fig(case + " gn planes from conv statistics vs fp64", ((nh.float() + nl.float()).double().cpu() - refn).abs().max().item(), 1e-4)
        e_ref = ((rh.float() + rl.float()).double().cpu() - refn).abs().max().item()
        assert e_pre < 1e-4 and e_pre < 1.5 * e_ref + 1e-6, (e_pre, e_ref)


@pytest.mark.parametrize("N,Cin,H,W,Co", [(2, 64, 8, 8, 64), (2, 64, 5, 5, 64)])
def test_subpixel_fallback(N, Cin, H, W, Co):
    """shapes the sub-pixel form does not take (H W below / no multiple of the tile) keep the gather form"""
    x, w, b = inputs(N, Cin, H, W, Co, 740)
    ok, y, _ = run(x, w, b, BF)
    assert not ok
    check(y, ref64(x, w, b, BF), BF, f"gather-form upsample conv {N}x{Cin}x{H}x{W}")


def test_subpixel_wrong_form_raises():
    """upsample2x = 2 with a residual is an error, not a silent fallback"""
    from cremage_amd import _lib as L
    from cremage_amd import ops
    dev = _dev()
    N, Cin, H, W, Co = 1, 64, 16, 16, 64
    x, w, b = inputs(N, Cin, H, W, Co, 760)
    xs = nhwc(x, BF)
    hi, _ = ops.packed_weight(w.to(dev), L.PACK_CONV_UP2, False)
    y = ops.empty_image(N, Co, 2 * H, 2 * W, BF, dev)
    res = torch.zeros_like(y)
    bias = b.to(dev)
    a = L.ConvArgs(x=xs.data_ptr(), x2=None, C1=Cin, C2=0, w=hi.data_ptr(), w_lo=None, bias=bias.data_ptr(), cvec=None, cvec_ld=0,
                   residual=res.data_ptr(), y=y.data_ptr(), N=N, H=H, W=W, Cout=Co, Ho=2 * H, Wo=2 * W, ksize=3, stride=1, pad_t=1, pad_l=1,
                   upsample2x=2, x_dtype=L.BF16, y_dtype=L.BF16, prec=L.PREC_BF16, x_lo=None)
    h = ops._h(xs)
    with pytest.raises(L.CrgError):
        L.check(L.load().crg_conv2d(h, ops._st(), C.byref(a)), h, "crg_conv2d")
    a.residual = None  # the same call without it is the sub-pixel form
    L.check(L.load().crg_conv2d(h, ops._st(), C.byref(a)), h, "crg_conv2d")
    check(y, ref64(x, w, b, BF), BF, "direct sub-pixel call")


def test_unet_upsample_keeps_gather_form():
    """16-bit operands keep the gather form unless asked (ldm_hip.unet.Upsample does not ask): bit for bit its output on a shape the
    sub-pixel form would take"""
    from cremage_amd import ops
    from cremage_amd.ldm_hip.unet import Upsample
    dev = _dev()
    N, Cin, H, W, Co = 2, 64, 16, 16, 64
    x, w, b = inputs(N, Cin, H, W, Co, 780)
    up = Upsample(Cin, True).to(dev).to(BF)
    with torch.no_grad():
        up.conv.weight.copy_(w)
        up.conv.bias.copy_(b)
        xs = nhwc(x, BF)
        assert ops.upsample_subpixel_ok(xs, up.conv.weight)
        y = up(xs)
        gather = ops.conv2d(xs, up.conv.weight, up.conv.bias, upsample2x=True, gn_stats=True, subpixel=False)
        default = ops.conv2d(xs, up.conv.weight, up.conv.bias, upsample2x=True, gn_stats=True)
        sub = ops.conv2d(xs, up.conv.weight, up.conv.bias, upsample2x=True, gn_stats=True, subpixel=True)
    assert torch.equal(y, gather) and torch.equal(default, gather)
    assert not torch.equal(gather, sub), "the two forms round differently: equal bits mean `subpixel` changed nothing"
    check(y, ref64(x, w, up.conv.bias.float().cpu(), BF), BF, "UNet Upsample (gather form)")


CHILD_TIME_LIMIT = 60  # seconds; measured on MI355X: the child takes 4.5 (interpreter and library start, then 1.2 for the cases above)


def test_this_file_against_the_fp16_library():
    """the half-type TAPS = 2 arms of libcrg_hip_f16.so: the tests above in ONE child process with CRG_HALF=f16 (the library is chosen when
    cremage_amd is imported; same pattern and bounds / 8 as tests/test_hip_ops_f16.py).  In that child this test is deselected."""
    from tests.conftest import REPO
    from cremage_amd import _lib as L
    if L.HALF_F16:
        return  # this process already runs the fp16 library: the tests above were that run
    me = "tests/test_conv_subpixel.py"
    cmd = [sys.executable, "-m", "pytest", me, "-m", "gpu", "-q", "-rs", "-p", "no:cacheprovider",
           "--deselect", me + "::test_this_file_against_the_fp16_library"]
    r = subprocess.run(cmd, cwd=REPO, env=dict(os.environ, CRG_HALF="f16"), capture_output=True, text=True, timeout=CHILD_TIME_LIMIT)
    tail = r.stdout[-6000:] + r.stderr[-3000:]
    assert r.returncode == 0, tail
    summary = [ln for ln in r.stdout.splitlines() if re.search(r"\b\d+ passed\b", ln)][-1]
    print(f"\n[parity] fp16 library, sub-pixel upsample convs: {summary.strip()}")
    counts = {k: int(n) for n, k in re.findall(r"(\d+) (passed|failed|skipped|errors?|xfailed|xpassed|deselected)", summary)}
    assert counts == {"passed": len(CASES) + 4, "deselected": 1}, (counts, tail)
