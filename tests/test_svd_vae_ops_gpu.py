"""The frame-conv kernels of the video VAE decoder (cremage_amd/csrc/video_x3.hip) through `cremage_amd.ops`: conv_frames_x3 (fp32 class
on pre-split planes) and conv_frames_thin (C <= 8 channels).

References are float64 torch on the CPU from the fp32 inputs; the bounds are `check` of tests/test_svd_ops_gpu.py in its fp32 class:
rel-L2 5e-5 and max-abs scale * 1e-4 + 1e-5 - in both builds (the fp16 build carries the planes as fp16: more mantissa, not less).
conv_frames_thin in fp32 is compared EXACTLY: the kernel is a chain of single fp32 FMAs in a documented order (bias, then taps -1, 0, +1,
input channels ascending), and `_fma32` below evaluates that chain with one correct rounding per FMA (the product of two fp32 values is
exact in float64; the float64 sum is corrected where it lands on an fp32 rounding tie, so no double rounding is left) - the order
argument holds, no tolerance is used.  The shapes live in tests/_svd_vae_cases.py, where tests/test_svd_vae_cpu.py holds every address
the kernels generate for them inside its operand."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests._svd_vae_cases import THIN_CASES, X3_CASES
from tests.test_hip_ops import BF, _dev, rnd
from tests.test_svd_ops_gpu import _conv_ref, check

pytestmark = pytest.mark.gpu
F32 = torch.float32


def _ops():
    from cremage_amd import ops
    return ops


def _planes(x):
    """fp32 tokens [F, S, C] on the device -> the (hi, lo) token planes, through crg_split_bf16 (the format group_norm(split=True) writes)"""
    ops = _ops()
    F, S, C = x.shape
    hi, lo = ops.split_bf16(ops.image_of(x, S, 1))
    return ops.tokens_of(hi), ops.tokens_of(lo)


def _inputs(b, T, S, Cin, Cout, gain=1.0):
    F = b * T
    x = rnd(F, S, Cin, seed=910) * gain
    w = rnd(Cout, Cin, 3, 1, 1, seed=911) * (3 * Cin) ** -0.5 * gain
    bias = rnd(Cout, seed=912) * gain
    cvec = rnd(F, Cout, seed=913) * gain
    res = rnd(F, S, Cout, seed=914) * gain
    rscale = torch.rand(F, generator=torch.Generator().manual_seed(915)) + 0.25
    rscale[F // 2] = 0.0
    return x, w, bias, cvec, res, rscale


def _x3(xd, wd, bd, T, **kw):
    hi, lo = _planes(xd)
    return _ops().conv_frames_x3(hi, lo, wd, bd, frames=T, **kw)


@pytest.mark.parametrize("gain", [1.0, 30.0], ids=["unit", "x30"])
@pytest.mark.parametrize("b,T,S,Cin,Cout", X3_CASES)
def test_conv_frames_x3(b, T, S, Cin, Cout, gain):
    dev = _dev()
    x, w, bias, cvec, res, rscale = _inputs(b, T, S, Cin, Cout, gain)
    xd, wd, bd, cd, rd, sd = (t.to(dev) for t in (x, w, bias, cvec, res, rscale))
    tag = f"conv_frames_x3 b{b} T{T} S{S} {Cin}->{Cout} x{gain:g}"
    x64, w64, b64 = x.double(), w.double(), bias.double()
    hi, lo = _planes(xd)
    run = lambda *a, **kw: _ops().conv_frames_x3(hi, lo, wd, *a, frames=T, **kw)
    check(run(None), _conv_ref(x64, w64, torch.zeros(Cout, dtype=torch.float64), T), F32, tag + " no bias")
    check(run(bd), _conv_ref(x64, w64, b64, T), F32, tag + " plain")
    check(run(bd, cvec=cd), _conv_ref(x64, w64, b64, T, cvec.double()), F32, tag + " cvec")
    check(run(bd, residual=rd), _conv_ref(x64, w64, b64, T, None, res.double()), F32, tag + " residual")
    got = run(bd, residual=rd, rscale=sd)
    check(got, _conv_ref(x64, w64, b64, T, None, res.double(), rscale.double()), F32, tag + " residual + rscale")
    f0 = (b * T) // 2  # rscale 0 there: the output IS the residual
    assert torch.equal(got[f0].cpu(), res[f0])
    full = run(bd, cvec=cd, residual=rd, rscale=sd)
    check(full, _conv_ref(x64, w64, b64, T, cvec.double(), res.double(), rscale.double()), F32, tag + " cvec + residual")
    assert full.dtype == F32 and full.shape == (b * T, S, Cout)
    # y aliasing the residual: the same bits, written in place
    buf = rd.clone()
    out = run(bd, cvec=cd, residual=buf, rscale=sd, out=buf)
    assert out.data_ptr() == buf.data_ptr() and torch.equal(buf, full)


@pytest.mark.parametrize("b,T,S,Cin,Cout", X3_CASES)
def test_conv_frames_x3_matches_the_composed_route(b, T, S, Cin, Cout):
    """the composed fp32 arm of ops.conv_frames (per video three row-shifted fp32-class GEMMs) on the same inputs: both within the fp32-class
    bound of the float64 reference, and of each other"""
    dev = _dev()
    x, w, bias, cvec, res, rscale = _inputs(b, T, S, Cin, Cout)
    xd, wd, bd, cd, rd, sd = (t.to(dev) for t in (x, w, bias, cvec, res, rscale))
    new = _x3(xd, wd, bd, T, cvec=cd, residual=rd, rscale=sd)
    old = _ops().conv_frames(xd, wd, bd, frames=T, cvec=cd, residual=rd, rscale=sd)
    tag = f"conv_frames_x3 vs composed b{b} T{T} S{S} {Cin}->{Cout}"
    check(new, old.double().cpu(), F32, tag)
    check(old, _conv_ref(x.double(), w.double(), bias.double(), T, cvec.double(), res.double(), rscale.double()), F32, tag + " (composed vs f64)")


@pytest.mark.parametrize("b,T,S,Cin,Cout", [(1, 3, 129, 128, 128), (1, 2, 1, 96, 32), (1, 5, 200, 256, 128)])
def test_conv_frames_x3_isolation_and_batch_position(b, T, S, Cin, Cout):
    """All-NaN videos in front of and behind the compared one: its output is finite and the bits of its stand-alone run.  A kernel that
    reads the neighbour video's rows and multiplies them by a zero mask fails this (0 * NaN).  And video 0 of two equals video 0 alone."""
    dev = _dev()
    x, w, bias, cvec, res, rscale = _inputs(1, T, S, Cin, Cout)
    xd, wd, bd, cd, rd, sd = (t.to(dev) for t in (x, w, bias, cvec, res, rscale))
    solo = _x3(xd, wd, bd, T, cvec=cd, residual=rd, rscale=sd)
    nan = torch.full_like(xd, float("nan"))
    three = lambda t: torch.cat([t, t, t])
    both = _x3(torch.cat([nan, xd, nan]), wd, bd, T, cvec=three(cd), residual=three(rd), rscale=three(sd))
    assert torch.isfinite(both[T:2 * T]).all()
    assert torch.equal(both[T:2 * T], solo)
    x2 = torch.cat([xd, xd.flip(0) * 0.5])
    pair = _x3(x2, wd, bd, T, cvec=torch.cat([cd, cd]), residual=torch.cat([rd, rd]), rscale=torch.cat([sd, sd]))
    assert torch.equal(pair[:T], solo)


def test_conv_frames_x3_batch_invariant_mode():
    """the same with the batch-invariant mode on: the tile shape comes from Cout alone either way"""
    import cremage_amd
    b, T, S, Cin, Cout = 1, 3, 129, 128, 128
    dev = _dev()
    x, w, bias, _, _, _ = _inputs(b, T, S, Cin, Cout)
    xd, wd, bd = x.to(dev), w.to(dev), bias.to(dev)
    solo_off = _x3(xd, wd, bd, T)
    cremage_amd.set_batch_invariant(8)
    try:
        solo = _x3(xd, wd, bd, T)
        pair = _x3(torch.cat([xd, xd * 2.0]), wd, bd, T)
    finally:
        cremage_amd.set_batch_invariant(0)
    assert torch.equal(solo, solo_off) and torch.equal(pair[:T], solo)


def test_conv_frames_x3_rejects():
    """each is refused on the host with CrgError: no launch (the output tensor is never created, the planes are untouched)"""
    ops, dev = _ops(), _dev()
    from cremage_amd._lib import CrgError
    pl = lambda F, S, C: torch.zeros(F, S, C, dtype=BF, device=dev)
    w = torch.zeros(32, 32, 3, 1, 1, device=dev)
    with pytest.raises(CrgError):  # Cin not a multiple of 32
        ops.conv_frames_x3(pl(4, 8, 48), pl(4, 8, 48), torch.zeros(32, 48, 3, 1, 1, device=dev), None, frames=2)
    with pytest.raises(CrgError):  # rscale without a residual
        ops.conv_frames_x3(pl(4, 8, 32), pl(4, 8, 32), w, None, frames=2, rscale=torch.ones(4, device=dev))
    with pytest.raises(CrgError):  # plane shape mismatch
        ops.conv_frames_x3(pl(4, 8, 32), pl(4, 9, 32), w, None, frames=2)
    with pytest.raises(CrgError):  # fp32 handed in as a plane
        ops.conv_frames_x3(pl(4, 8, 32).float(), pl(4, 8, 32), w, None, frames=2)
    with pytest.raises(CrgError):  # 4 frames are no whole number of 3-frame videos
        ops.conv_frames_x3(pl(4, 8, 32), pl(4, 8, 32), w, None, frames=3)
    with pytest.raises(CrgError):  # half-type residual
        ops.conv_frames_x3(pl(4, 8, 32), pl(4, 8, 32), w, None, frames=2, residual=pl(4, 8, 32))
    # the library's own argument check (reached past the Python arm): -22, no launch
    from cremage_amd import _lib as L
    import ctypes as C
    z = pl(4, 8, 32)
    y = torch.zeros(4, 8, 32, device=dev)
    a = L.ConvFramesX3Args(x_hi=z.data_ptr(), x_lo=z.data_ptr(), w_hi=z.data_ptr(), w_lo=z.data_ptr(), y=y.data_ptr(), b=2, T=2, S=8, Cin=48, Cout=32)
    assert L.load().crg_conv_frames_x3(L.ctx(0), None, C.byref(a)) == -22
    a = L.ConvFramesX3Args(x_hi=z.data_ptr(), x_lo=z.data_ptr(), w_hi=z.data_ptr(), w_lo=z.data_ptr(), y=y.data_ptr(), b=2, T=2, S=8, Cin=32, Cout=32,
                           rscale=y.data_ptr())
    assert L.load().crg_conv_frames_x3(L.ctx(0), None, C.byref(a)) == -22
    # y overlapping an activation plane, or the residual at an offset (exactly the residual is allowed)
    big = torch.zeros(2 * 4 * 8 * 32, device=dev)
    a = L.ConvFramesX3Args(x_hi=big.data_ptr(), x_lo=z.data_ptr(), w_hi=z.data_ptr(), w_lo=z.data_ptr(), y=big.data_ptr() + 64, b=2, T=2, S=8,
                           Cin=32, Cout=32)
    assert L.load().crg_conv_frames_x3(L.ctx(0), None, C.byref(a)) == -22
    a = L.ConvFramesX3Args(x_hi=z.data_ptr(), x_lo=z.data_ptr(), w_hi=z.data_ptr(), w_lo=z.data_ptr(), y=big.data_ptr() + 64, residual=big.data_ptr(),
                           b=2, T=2, S=8, Cin=32, Cout=32)
    assert L.load().crg_conv_frames_x3(L.ctx(0), None, C.byref(a)) == -22
    assert not big.any()  # nothing was launched


# ------------------------------------------------------------------------------------------------------------------ conv_frames_thin
def _fma32(a, b, c):
    """fp32 fma(a, b, c) with ONE rounding, on numpy float32 arrays: the product is exact in float64; the float64 sum s = p + c has the
    exact error e (TwoSum); float32(s) is the correctly rounded result unless s sits exactly on a tie between two fp32 values and e != 0,
    where the true value lies on e's side of the tie."""
    p = a.astype(np.float64) * b.astype(np.float64)
    c64 = c.astype(np.float64)
    s = p + c64
    bb = s - p
    e = (p - (s - bb)) + (c64 - bb)
    r = s.astype(np.float32)
    r64 = r.astype(np.float64)
    up, dn = np.nextafter(r, np.float32(np.inf)), np.nextafter(r, np.float32(-np.inf))
    tie_up = (r64 < s) & (s - r64 == up.astype(np.float64) - s)   # r below s, s the midpoint of (r, up)
    tie_dn = (r64 > s) & (r64 - s == s - dn.astype(np.float64))   # r above s, s the midpoint of (dn, r)
    r = np.where(tie_up & (e > 0), up, r)
    r = np.where(tie_dn & (e < 0), dn, r)
    return r.astype(np.float32)


def _thin_ref(x, w, bias, T):
    """x [F, S, C] float32 numpy, w [C, C, 3], bias [C] or None -> the kernel's FMA chain, evaluated with exactly rounded FMAs"""
    F, S, C = x.shape
    xv = x.reshape(F // T, T, S, C)
    acc = np.broadcast_to((bias if bias is not None else np.zeros(C, np.float32)).astype(np.float32), (F // T, T, S, C)).copy()
    for d in range(3):
        lo, hi = max(0, 1 - d), min(T, T + 1 - d)  # frames t with 0 <= t + d - 1 < T
        if lo >= hi:
            continue
        src = xv[:, lo + d - 1:hi + d - 1]
        for ci in range(C):
            for co in range(C):
                acc[:, lo:hi, :, co] = _fma32(np.broadcast_to(w[co, ci, d], src[..., ci].shape), src[..., ci], acc[:, lo:hi, :, co])
    return acc.reshape(F, S, C)


def _thin_inputs(b, T, S, C):
    x = rnd(b * T, S, C, seed=920)
    w = rnd(C, C, 3, 1, 1, seed=921) * (3 * C) ** -0.5
    bias = rnd(C, seed=922)
    return x, w, bias


@pytest.mark.parametrize("b,T,S,C", THIN_CASES)
def test_conv_frames_thin(b, T, S, C):
    ops, dev = _ops(), _dev()
    x, w, bias = _thin_inputs(b, T, S, C)
    for bb in (bias, None):
        got = ops.conv_frames_thin(x.to(dev), w.to(dev), bb.to(dev) if bb is not None else None, frames=T)
        ref = _thin_ref(x.numpy(), w.reshape(C, C, 3).numpy(), bb.numpy() if bb is not None else None, T)
        assert got.dtype == F32 and got.shape == x.shape
        assert np.array_equal(got.cpu().numpy(), ref), (np.abs(got.cpu().numpy() - ref).max(), b, T, S, C)  # exact
    # half type: fp32 arithmetic on the rounded input, one rounding of the result
    xh = x.to(BF)
    got = ops.conv_frames_thin(xh.to(dev), w.to(dev), bias.to(dev), frames=T)
    assert got.dtype == BF
    w5 = torch.zeros(C, C, 3, 1, 1, dtype=torch.float64)
    w5[:] = w.double()
    check(got, _conv_ref_thin(xh.double(), w5, bias.double(), T), BF, f"conv_frames_thin half b{b} T{T} S{S} C{C}")


def _conv_ref_thin(x, w, bias, T):
    return _conv_ref(x, w, bias, T)


@pytest.mark.parametrize("T,S", [(T, S) for T in (1, 2, 5) for S in (1, 129)])
def test_conv_frames_thin_isolation(T, S):
    ops, dev = _ops(), _dev()
    C = 3
    x, w, bias = _thin_inputs(1, T, S, C)
    xd, wd, bd = x.to(dev), w.to(dev), bias.to(dev)
    solo = ops.conv_frames_thin(xd, wd, bd, frames=T)
    nan = torch.full_like(xd, float("nan"))
    both = ops.conv_frames_thin(torch.cat([nan, xd, nan]), wd, bd, frames=T)
    assert torch.isfinite(both[T:2 * T]).all() and torch.equal(both[T:2 * T], solo)
    assert torch.equal(ops.conv_frames_thin(torch.cat([xd, xd * 3.0]), wd, bd, frames=T)[:T], solo)


def test_conv_frames_thin_rejects():
    ops, dev = _ops(), _dev()
    from cremage_amd._lib import CrgError
    with pytest.raises(CrgError):
        ops.conv_frames_thin(torch.zeros(4, 8, 9, device=dev), torch.zeros(9, 9, 3, 1, 1, device=dev), None, frames=2)
    with pytest.raises(CrgError):
        ops.conv_frames_thin(torch.zeros(4, 8, 3, device=dev), torch.zeros(3, 4, 3, 1, 1, device=dev), None, frames=2)
    with pytest.raises(CrgError):
        ops.conv_frames_thin(torch.zeros(4, 8, 3, device=dev), torch.zeros(3, 3, 3, 1, 1, device=dev), None, frames=3)
    # the library's own check: y overlapping x at any offset is refused (-22), x itself included
    from cremage_amd import _lib as L
    buf = torch.ones(2 * 4 * 8 * 3, device=dev)
    w = torch.ones(3, 3, 3, device=dev)
    P = C.c_void_p
    for off in (0, 12, 4 * (4 * 8 * 3 - 1)):
        rc = L.load().crg_conv_frames_thin(L.ctx(0), None, P(buf.data_ptr()), P(w.data_ptr()), None, P(buf.data_ptr() + off), 2, 2, 8, 3, L.F32)
        assert rc == -22, off
    assert bool((buf == 1).all())


# ------------------------------------------------------------------------------------------------------------------ the fp16 build
N_TESTS = 10 + 5 + 3 + 1 + 1 + 12 + 6 + 1  # cases of this file without the test below
CHILD_TIME_LIMIT = 120                     # seconds


def test_this_file_against_the_fp16_library():
    """the same cases in ONE child process with CRG_HALF=f16 (the pattern of tests/test_svd_ops_gpu.py).  In that child this test is
    deselected."""
    from tests.conftest import REPO
    from cremage_amd import _lib as L
    if L.HALF_F16:
        return  # this process already runs the fp16 library: the tests above were that run
    me = "tests/test_svd_vae_ops_gpu.py"
    cmd = [sys.executable, "-m", "pytest", me, "-m", "gpu", "-q", "-rs", "-p", "no:cacheprovider",
           "--deselect", me + "::test_this_file_against_the_fp16_library"]
    r = subprocess.run(cmd, cwd=REPO, env=dict(os.environ, CRG_HALF="f16"), capture_output=True, text=True, timeout=CHILD_TIME_LIMIT)
    tail = r.stdout[-6000:] + r.stderr[-3000:]
    assert r.returncode == 0, tail
    summary = [ln for ln in r.stdout.splitlines() if re.search(r"\b\d+ passed\b", ln)][-1]
    print(f"\n[parity] fp16 library, video VAE kernels: {summary.strip()}")
    counts = {k: int(n) for n, k in re.findall(r"(\d+) (passed|failed|skipped|errors?|xfailed|xpassed|deselected)", summary)}
    assert counts == {"passed": N_TESTS, "deselected": 1}, (counts, tail)
