"""The temporal kernels of the video UNet (cremage_amd/csrc/video.hip) through `cremage_amd.ops`: conv_frames, attention_frames and the
per-frame add / blend.

References are float64 torch on the CPU, computed from inputs rounded to the storage type.  Bounds are those of
tests/test_hip_ops.py::check, restated: half type rel-L2 6e-3 * HS and max-abs (scale * 2^-6 + 1e-3) * HS, fp32 class rel-L2 5e-5 (and
its max-abs scale * 1e-4 + 1e-5), HS = 2^-3 in the fp16 build.  The shapes live in tests/_svd_cases.py, where tests/test_svd_cpu.py
holds every address the kernels generate for them inside its operand."""
import os
import re
import subprocess
import sys

import pytest
import torch

from tests._svd_cases import ATTN_CASES, CONV_CASES
from tests.test_hip_ops import BF, HS, _dev, fig, rnd

pytestmark = pytest.mark.gpu

DTYPES = [BF, torch.float32]


def check(got, ref, dtype, what=""):  # tests/test_hip_ops.py::check on a float64 reference
    got = got.detach().double().cpu()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert torch.isfinite(got).all(), what
    rel = ((got - ref).norm() / ref.norm().clamp_min(1e-20)).item()
    mx = (got - ref).abs().max().item()
    scale = ref.abs().max().item()
    b_rel, b_mx = (6e-3 * HS, (scale * 2 ** -6 + 1e-3) * HS) if dtype == BF else (5e-5, scale * 1e-4 + 1e-5)
    fig(what + " rel-L2", rel, b_rel)
    fig(what + " max-abs", mx, b_mx)
    assert rel < b_rel and mx < b_mx, (what, rel, mx, scale)


def _ops():
    from cremage_amd import ops
    return ops


# ---------------------------------------------------------------------------------------------------------------------- conv_frames
def _conv_ref(x, w, bias, T, cvec=None, residual=None, rscale=None):
    """x [F, S, Cin], w [Cout, Cin, 3, 1, 1], all float64"""
    F, S, Cin = x.shape
    xv = x.reshape(F // T, T, S, Cin)
    w3 = w.reshape(w.shape[0], Cin, 3)
    y = torch.einsum("btsc,oc->btso", xv, w3[:, :, 1])
    if T > 1:
        y[:, 1:] += torch.einsum("btsc,oc->btso", xv[:, :-1], w3[:, :, 0])
        y[:, :-1] += torch.einsum("btsc,oc->btso", xv[:, 1:], w3[:, :, 2])
    y = y.reshape(F, S, -1) + bias
    if cvec is not None:
        y = y + cvec[:, None, :]
    if residual is not None:
        y = residual + (rscale[:, None, None] if rscale is not None else 1.0) * y
    return y


def _conv_inputs(b, T, S, Cin, Cout, dtype):
    F = b * T
    x = rnd(F, S, Cin, seed=810).to(dtype)
    w = (rnd(Cout, Cin, 3, 1, 1, seed=811) * (3 * Cin) ** -0.5)
    w = w.to(dtype).float() if dtype == BF else w  # the half route multiplies by the half-rounded weight; parameters stay fp32 tensors
    bias = rnd(Cout, seed=812)
    cvec = rnd(F, Cout, seed=813)
    res = rnd(F, S, Cout, seed=814).to(dtype)
    rscale = torch.rand(F, generator=torch.Generator().manual_seed(815)) + 0.25
    rscale[F // 2] = 0.0
    return x, w, bias, cvec, res, rscale


@pytest.mark.parametrize("dtype", DTYPES, ids=["half", "fp32"])
@pytest.mark.parametrize("b,T,S,Cin,Cout", CONV_CASES)
def test_conv_frames(b, T, S, Cin, Cout, dtype):
    ops, dev = _ops(), _dev()
    x, w, bias, cvec, res, rscale = _conv_inputs(b, T, S, Cin, Cout, dtype)
    xd, wd, bd, cd, rd, sd = (t.to(dev) for t in (x, w, bias, cvec, res, rscale))
    tag = f"conv_frames b{b} T{T} S{S} {Cin}->{Cout}"
    x64, w64, b64 = x.double(), w.double(), bias.double()
    check(ops.conv_frames(xd, wd, bd, frames=T), _conv_ref(x64, w64, b64, T), dtype, tag + " plain")
    check(ops.conv_frames(xd, wd, bd, frames=T, cvec=cd), _conv_ref(x64, w64, b64, T, cvec.double()), dtype, tag + " cvec")
    got = ops.conv_frames(xd, wd, bd, frames=T, residual=rd, rscale=sd)
    check(got, _conv_ref(x64, w64, b64, T, None, res.double(), rscale.double()), dtype, tag + " residual")
    f0 = (b * T) // 2  # rscale 0 there: the output IS the residual
    assert torch.equal(got[f0].cpu(), res[f0])
    got = ops.conv_frames(xd, wd, bd, frames=T, cvec=cd, residual=rd, rscale=sd)
    check(got, _conv_ref(x64, w64, b64, T, cvec.double(), res.double(), rscale.double()), dtype, tag + " cvec + residual")
    assert got.dtype == dtype and got.shape == (b * T, S, Cout)


@pytest.mark.parametrize("dtype", DTYPES, ids=["half", "fp32"])
@pytest.mark.parametrize("b,T,S,Cin,Cout", CONV_CASES)
def test_conv_frames_isolation(b, T, S, Cin, Cout, dtype):
    """Video 1 is NaN: video 0's output is finite and the bits of its solo run.  A kernel that reads the neighbour video's rows and
    multiplies them by a zero mask fails this (0 * NaN)."""
    ops, dev = _ops(), _dev()
    x, w, bias, cvec, _, _ = _conv_inputs(1, T, S, Cin, Cout, dtype)
    xd, wd, bd, cd = (t.to(dev) for t in (x, w, bias, cvec))
    solo = ops.conv_frames(xd, wd, bd, frames=T, cvec=cd)
    both = ops.conv_frames(torch.cat([xd, torch.full_like(xd, float("nan"))]), wd, bd, frames=T, cvec=torch.cat([cd, cd]))
    assert torch.isfinite(both[:T]).all()
    assert torch.equal(both[:T], solo)
    # and with the NaN video in front: the frame before video 1's first one is never read either
    both = ops.conv_frames(torch.cat([torch.full_like(xd, float("nan")), xd]), wd, bd, frames=T, cvec=torch.cat([cd, cd]))
    assert torch.equal(both[T:], solo)


def test_conv_frames_rejects():
    ops, dev = _ops(), _dev()
    from cremage_amd._lib import CrgError
    x = torch.zeros(4, 8, 32, dtype=BF, device=dev)
    w = torch.zeros(32, 32, 3, 1, 1, device=dev)
    with pytest.raises(CrgError):
        ops.conv_frames(x, w, None, frames=3)  # 4 frames are no whole number of 3-frame videos
    with pytest.raises(CrgError):
        ops.conv_frames(x, torch.zeros(48, 32, 3, 1, 1, device=dev), None, frames=2)  # Cout % 32
    with pytest.raises(CrgError):
        ops.conv_frames(x, w, None, frames=2, rscale=torch.ones(4, device=dev))  # rscale without a residual


# ----------------------------------------------------------------------------------------------------------------- attention_frames
def _attn_ref(q, k, v, heads, T, scale):
    """q, k, v [F, S, C] float64 -> softmax over the T frames of each (video, pixel, head)"""
    F, S, C = q.shape
    sp = lambda t: t.reshape(F // T, T, S, heads, C // heads).permute(0, 2, 3, 1, 4)  # [b, S, H, T, d]
    p = torch.softmax(sp(q) @ sp(k).transpose(-1, -2) * scale, dim=-1)
    return (p @ sp(v)).permute(0, 3, 1, 2, 4).reshape(F, S, C)


def _qkv(b, T, S, heads, d, dtype, gain=1.0):
    return (rnd(b * T, S, 3 * heads * d, seed=820) * gain).to(dtype)


def _run_attn(qkv, heads, T):
    ops = _ops()
    C = qkv.shape[-1] // 3
    dv = qkv.to(_dev())
    q, k, v = dv[..., :C], dv[..., C:2 * C], dv[..., 2 * C:]  # uncopied column slices of one [rows, 3C] tensor
    assert q.data_ptr() == dv.data_ptr() and not k.is_contiguous()
    return ops.attention_frames(q, k, v, heads, frames=T)


@pytest.mark.parametrize("dtype", DTYPES, ids=["half", "fp32"])
@pytest.mark.parametrize("b,T,S,heads,d", ATTN_CASES)
def test_attention_frames(b, T, S, heads, d, dtype):
    C = heads * d
    qkv = _qkv(b, T, S, heads, d, dtype)
    got = _run_attn(qkv, heads, T)
    q64 = qkv.double()
    ref = _attn_ref(q64[..., :C], q64[..., C:2 * C], q64[..., 2 * C:], heads, T, d ** -0.5)
    assert got.dtype == dtype and got.is_contiguous()
    check(got, ref, dtype, f"attention_frames b{b} T{T} S{S} h{heads} d{d}")
    if T == 1:  # one frame: the softmax is exactly 1 and the output is V
        assert torch.equal(got.cpu(), qkv[..., 2 * C:])


@pytest.mark.parametrize("dtype", DTYPES, ids=["half", "fp32"])
def test_attention_frames_large_logits(dtype):
    b, T, S, heads, d = 2, 25, 72, 5, 64
    C = heads * d
    qkv = _qkv(b, T, S, heads, d, dtype, gain=30.0)
    got = _run_attn(qkv, heads, T)
    q64 = qkv.double()
    check(got, _attn_ref(q64[..., :C], q64[..., C:2 * C], q64[..., 2 * C:], heads, T, d ** -0.5), dtype, "attention_frames x30")


@pytest.mark.parametrize("dtype", DTYPES, ids=["half", "fp32"])
def test_attention_frames_isolation(dtype):
    b, T, S, heads, d = 2, 3, 128, 2, 16
    qkv = _qkv(b, T, S, heads, d, dtype)
    solo = _run_attn(qkv[:T], heads, T)
    qkv[T:] = float("nan")
    both = _run_attn(qkv, heads, T)
    assert torch.isfinite(both[:T]).all() and torch.equal(both[:T], solo)


def test_attention_frames_too_many_frames():
    from cremage_amd._lib import CrgError
    with pytest.raises(CrgError):
        _run_attn(_qkv(1, 33, 4, 1, 16, BF), 1, 33)


# --------------------------------------------------------------------------------------------------------------- per-frame add / blend
def test_add_frames_exact():
    ops, dev = _ops(), _dev()
    F, S, C = 6, 37, 40
    x, e = rnd(F, S, C, seed=830), rnd(F, C, seed=831)
    assert torch.equal(ops.add_frames(x.to(dev), e.to(dev)).cpu(), x + e[:, None, :])
    xh, eh = x.to(BF), e.to(BF)
    check(ops.add_frames(xh.to(dev), eh.to(dev)), xh.double() + eh.double()[:, None, :], BF, "add_frames half")


def test_blend_frames_exact():
    """learned_with_images with a mixed image_only_indicator: alpha is 1 on the image-only frames and sigmoid(mix_factor) on the others"""
    ops, dev = _ops(), _dev()
    F, S, C = 6, 37, 40
    x, z = rnd(F, S, C, seed=832), rnd(F, S, C, seed=833)
    indicator = torch.tensor([1, 0, 0, 1, 0, 1], dtype=torch.bool)
    alpha = torch.where(indicator, torch.ones(()), torch.sigmoid(torch.tensor(0.5)))
    want = alpha[:, None, None] * x + (1.0 - alpha)[:, None, None] * z
    got = ops.blend_frames(alpha.to(dev), x.to(dev), z.to(dev)).cpu()
    assert torch.equal(got, want)
    assert torch.equal(got[indicator], x[indicator])  # image-only frames pass through
    xh, zh = x.to(BF), z.to(BF)
    ref = alpha.double()[:, None, None] * xh.double() + (1.0 - alpha).double()[:, None, None] * zh.double()
    check(ops.blend_frames(alpha.to(dev), xh.to(dev), zh.to(dev)), ref, BF, "blend_frames half")


# ------------------------------------------------------------------------------------------------------------------ the fp16 build
N_TESTS = 38           # cases of this file without the test below
CHILD_TIME_LIMIT = 90  # seconds; measured on MI355X: the 38 cases take 1.4 s after interpreter and library start


def test_this_file_against_the_fp16_library():
    """the same cases in ONE child process with CRG_HALF=f16 (the library is chosen when cremage_amd is imported; the pattern of
    tests/test_small_ops_gpu.py).  In that child this test is deselected."""
    from tests.conftest import REPO
    from cremage_amd import _lib as L
    if L.HALF_F16:
        return  # this process already runs the fp16 library: the tests above were that run
    me = "tests/test_svd_ops_gpu.py"
    cmd = [sys.executable, "-m", "pytest", me, "-m", "gpu", "-q", "-rs", "-p", "no:cacheprovider",
           "--deselect", me + "::test_this_file_against_the_fp16_library"]
    r = subprocess.run(cmd, cwd=REPO, env=dict(os.environ, CRG_HALF="f16"), capture_output=True, text=True, timeout=CHILD_TIME_LIMIT)
    tail = r.stdout[-6000:] + r.stderr[-3000:]
    assert r.returncode == 0, tail
    summary = [ln for ln in r.stdout.splitlines() if re.search(r"\b\d+ passed\b", ln)][-1]
    print(f"\n[parity] fp16 library, temporal kernels: {summary.strip()}")
    counts = {k: int(n) for n, k in re.findall(r"(\d+) (passed|failed|skipped|errors?|xfailed|xpassed|deselected)", summary)}
    assert counts == {"passed": N_TESTS, "deselected": 1}, (counts, tail)
