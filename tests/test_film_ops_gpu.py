"""The FILM kernels of film.hip against float64 truth computed on the host from their definitions (tests/_film_cases.py).

Criterion for the four data movements: the kernel's largest error is at most twice the largest error of the plain-torch fp32 restatement
against the same truth, plus one fp32 ulp of max |x| - the kernel is as accurate as the reference's own arithmetic, no tolerance is invented.
The convs go through the existing fp32-class route and are held to that route's parity bound (tests/test_hip_ops.py `check`) against
what the reference's util.Conv2d produced (`film_ops` fixture)."""
import math

import pytest
import torch
import torch.nn.functional as F

from tests import _film_cases as FC
from tests.conftest import load_golden

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL = 777.25


def _ulp(x: float) -> float:
    return 2.0 ** (math.floor(math.log2(x)) - 23) if x > 0 else 0.0


def _cl(x):
    """NCHW host tensor -> channels-last device tensor (a layout change only)"""
    return x.to(DEV).contiguous(memory_format=torch.channels_last)


def _as_accurate(what, got, restated, truth, scale):
    e_k = float((got.detach().double().cpu() - truth).abs().max())
    e_r = float((restated.double() - truth).abs().max())
    bound = 2 * e_r + _ulp(scale)
    print(f"[fig] {what}: kernel {e_k:.3e} restatement {e_r:.3e} bound {bound:.3e}")
    assert e_k <= bound, (what, e_k, e_r, bound)


def _slice_of(n, c, h, w, off=5, extra=9, dtype=torch.float32):
    """a [n, c, h, w] channel slice at offset `off` of a sentinel-filled buffer c + extra wide"""
    buf = torch.full((n, h, w, c + extra), SENTINEL, dtype=dtype, device=DEV).permute(0, 3, 1, 2)
    return buf, buf[:, off:off + c]


def _sentinels_survive(buf, off, c):
    assert bool((buf[:, :off] == SENTINEL).all()) and bool((buf[:, off + c:] == SENTINEL).all())


# ------------------------------------------------------------------------------------------------------------------------------- warp
@pytest.mark.parametrize("name,shape,amp,scales", FC.WARP_CASES, ids=[c[0] for c in FC.WARP_CASES])
def test_warp(name, shape, amp, scales):
    from cremage_amd import ops
    n, c, h, w = shape
    src, flow = FC.warp_case_inputs(name, shape, amp)
    s = None if scales is None else torch.tensor(scales, dtype=torch.float32)
    truth, restated = FC.warp_truth(src, flow, s), FC.warp(src, flow, s)
    if h * w > 2:  # the case really leaves the image on all four sides
        f = flow if s is None else flow * s.reshape(-1, 1, 1, 1)
        px, py = torch.arange(w)[None, None, :] + f[:, 0], torch.arange(h)[None, :, None] + f[:, 1]
        assert float(px.min()) < 0 and float(px.max()) > w - 1 and float(py.min()) < 0 and float(py.max()) > h - 1
    sd = None if s is None else s.to(DEV)
    got = ops.warp_flow(_cl(src), _cl(flow), sd)
    assert tuple(got.shape) == shape
    _as_accurate(name, got, restated, truth, float(src.abs().max()))
    _, fixture = load_golden("film_ops")
    _as_accurate(name + " (reference's own output)", got, fixture[name], truth, float(src.abs().max()))
    # destination: offset 5 in rows of C + 9; source: a non-contiguous view (the odd columns of a buffer twice as wide, plus one)
    buf, dst = _slice_of(n, c, h, w)
    wide = torch.full((n, h, w, 2 * c + 1), SENTINEL, device=DEV).permute(0, 3, 1, 2)
    wide[:, 1:1 + c] = src.to(DEV)
    out = ops.warp_flow(wide[:, 1:1 + c], _cl(flow), sd, out=dst)
    assert out.data_ptr() == dst.data_ptr() and torch.equal(dst, got)
    _sentinels_survive(buf, 5, c)
    # planes: hi + lo is the fp32 result to the split format's 2^-16
    _, (hi, lo) = ops.warp_flow(_cl(src), _cl(flow), sd, planes=True)
    rec = hi.float() + lo.float()
    assert float(((rec - got).abs() / got.abs().clamp_min(2.0 ** -100)).max()) <= 2.0 ** -16


@pytest.mark.parametrize("shape", [(2, 3, 5, 7), (2, 67, 5, 7), (1, 64, 1, 2), (2, 8, 6, 4)])
def test_warp_zero_and_integral_flow_is_exact(shape):
    from cremage_amd import ops
    n, c, h, w = shape
    src = FC.synth("warp_exact.src", shape)
    src[0, 0, 0, 0] = -0.0
    x = _cl(src)
    zero = torch.zeros((n, 2, h, w))
    got = ops.warp_flow(x, _cl(zero), torch.full((n,), 0.75, device=DEV))
    assert torch.equal(got.cpu().view(torch.int32), src.view(torch.int32))  # bit for bit
    # an integral shift with the border clamp: a gather of source pixels, exactly
    flow = torch.zeros((n, 2, h, w))
    flow[:, 0], flow[:, 1] = 2.0, -1.0
    got = ops.warp_flow(x, _cl(flow)).cpu()
    yy = (torch.arange(h) - 1).clamp(0, h - 1)
    xx = (torch.arange(w) + 2).clamp(0, w - 1)
    assert torch.equal(got, src[:, :, yy][:, :, :, xx])


def test_warp_rejects_what_it_cannot_address():
    from cremage_amd import ops
    from cremage_amd._lib import CrgError
    x = _cl(torch.zeros(1, 8, 4, 6))
    with pytest.raises(CrgError):
        ops.warp_flow(x, _cl(torch.zeros(1, 2, 4, 5)))
    with pytest.raises(CrgError):
        ops.warp_flow(x.contiguous(), _cl(torch.zeros(1, 2, 4, 6)))  # NCHW strides: not rows of channels
    with pytest.raises(CrgError):
        ops.warp_flow(x, _cl(torch.zeros(1, 2, 4, 6)), out=torch.empty((1, 4, 6, 7), device=DEV).permute(0, 3, 1, 2))
    with pytest.raises(CrgError):
        ops.warp_flow(torch.zeros(1, 8, 4, 6), torch.zeros(1, 2, 4, 6))


# ------------------------------------------------------------------------------------------------------------------------------- pool
@pytest.mark.parametrize("name,shape", FC.POOL_CASES, ids=[c[0] for c in FC.POOL_CASES])
def test_avg_pool2(name, shape):
    from cremage_amd import ops
    n, c, h, w = shape
    x = FC.synth(name + ".x", shape)
    truth = F.avg_pool2d(x.double(), 2, 2)
    assert tuple(truth.shape) == (n, c, h // 2, w // 2)
    buf, dst = _slice_of(n, c, h // 2, w // 2)
    ops.avg_pool2(_cl(x), out=dst)
    _as_accurate(name, dst, FC.avg_pool2(x), truth, float(x.abs().max()))
    _sentinels_survive(buf, 5, c)
    assert torch.equal(ops.avg_pool2(_cl(x)), dst)
    _, fixture = load_golden("film_ops")
    _as_accurate(name + " (reference's own output)", dst, fixture[name], truth, float(x.abs().max()))


# ------------------------------------------------------------------------------------------------------------------------------- flow upsampling
@pytest.mark.parametrize("with_res", [False, True])
@pytest.mark.parametrize("name,shape", FC.UP_CASES, ids=[c[0] for c in FC.UP_CASES])
def test_flow_up2_add(name, shape, with_res):
    from cremage_amd import ops
    n, _, h, w = shape
    v = FC.synth(name + ".v", shape, 3.0)
    res = FC.synth(name + ".res", (n, 2, 2 * h, 2 * w)) if with_res else None
    truth, restated = FC.flow_up2_truth(v, res), FC.flow_up2_add(v, res)
    got = ops.flow_up2_add(_cl(v), None if res is None else _cl(res))
    assert tuple(got.shape) == (n, 2, 2 * h, 2 * w)
    scale = float((2 * v).abs().max())
    edge = torch.zeros((2 * h, 2 * w), dtype=torch.bool)  # where the source index clamps
    edge[0], edge[-1], edge[:, 0], edge[:, -1] = True, True, True, True
    for what, m in (("edge", edge), ("interior", ~edge)):
        if bool(m.any()):
            _as_accurate(f"{name} res={with_res} {what}", got.cpu()[:, :, m], restated[:, :, m], truth[:, :, m], scale)
    _, fixture = load_golden("film_ops")
    _as_accurate(name + " (reference's own output)", got, fixture[name + ("_res" if with_res else "")], truth, scale)
    buf, dst = _slice_of(n, 2, 2 * h, 2 * w)
    ops.flow_up2_add(_cl(v), None if res is None else _cl(res), out=dst)
    assert torch.equal(dst, got)
    _sentinels_survive(buf, 5, 2)


# ------------------------------------------------------------------------------------------------------------------------------- LeakyReLU
@pytest.mark.parametrize("shape", [(2, 24, 6, 10), (2, 3, 7, 9), (1, 67, 5, 7), (2, 64, 2, 2)])
def test_leaky_split(shape):
    from cremage_amd import ops
    n, c, h, w = shape
    x = FC.synth("leaky.x", shape, 2.0)
    x[0, 0].view(-1)[:4] = torch.tensor([-1.0, -0.0, 0.0, 1.0])  # the sign boundary
    truth = F.leaky_relu(x.double(), 0.2)
    buf, dst = _slice_of(n, c, h, w)
    hbuf, hdst = _slice_of(n, c, h, w, dtype=ops.HALF)
    lbuf, ldst = _slice_of(n, c, h, w, dtype=ops.HALF)
    y, planes, pooled = ops.leaky_split(_cl(x), 0.2, out=dst, planes=(hdst, ldst), pool=True)
    assert y.data_ptr() == dst.data_ptr()
    _as_accurate(f"leaky {shape}", y, FC.leaky(x), truth, float(x.abs().max()))
    got = y.cpu()
    assert got[0, 0].reshape(-1)[:4].tolist() == [float(torch.tensor(-1.0) * torch.tensor(0.2)), 0.0, 0.0, 1.0]
    for b in (buf, hbuf, lbuf):
        _sentinels_survive(b, 5, c)
    rec = planes[0].float() + planes[1].float()
    assert float(((rec - y).abs() / y.abs().clamp_min(2.0 ** -100)).max()) <= 2.0 ** -16
    # the fused 2 x 2 mean is avg_pool2 of the unfused activation, to the bit
    alone, _, _ = ops.leaky_split(_cl(x), 0.2)
    assert torch.equal(alone, y)
    assert torch.equal(pooled, ops.avg_pool2(alone)) and tuple(pooled.shape) == (n, c, h // 2, w // 2)
    # in place, planes only, and the per-sample scale behind the activation
    xi = _cl(x).clone(memory_format=torch.preserve_format)
    assert ops.leaky_split(xi, 0.2, out=xi)[0] is xi and torch.equal(xi, y)
    _, only, _ = ops.leaky_split(_cl(x), 0.2, fp32=False, planes=True)
    assert torch.equal(only[0], planes[0]) and torch.equal(only[1], planes[1])
    s = torch.tensor([0.5, 0.75][:n])
    scaled = ops.scale_into(_cl(x), s.to(DEV), out=torch.empty_like(y))
    assert torch.equal(scaled.cpu(), x * s.reshape(-1, 1, 1, 1))


# ------------------------------------------------------------------------------------------------------------------------------- convs
def _check_conv(got, ref, what):
    """the fp32-class arm of tests/test_hip_ops.py `check`"""
    got, ref = got.detach().float().cpu(), ref.float()
    assert got.shape == ref.shape and bool(torch.isfinite(got).all()), what
    rel = float((got - ref).norm() / ref.norm().clamp_min(1e-20))
    mx, scale = float((got - ref).abs().max()), float(ref.abs().max())
    print(f"[fig] {what}: rel-L2 {rel:.3e} (bound 5e-5) max-abs {mx:.3e} (bound {scale * 1e-4 + 1e-5:.3e})")
    assert rel < 5e-5 and mx < scale * 1e-4 + 1e-5, (what, rel, mx, scale)


@pytest.mark.parametrize("name,cin,cout,k,act", FC.CONV_CASES, ids=[c[0] for c in FC.CONV_CASES])
def test_film_conv_shapes(name, cin, cout, k, act):
    """every shape class of a FILM conv through the layout the model uses: input channels that are 2 mod 8 sit in a buffer rounded up to a
    multiple of 8 with zeroed slots (and zero weight columns), the 2 x 2 conv is a 3 x 3 one with embedded taps"""
    from cremage_amd import ops
    from cremage_amd.film_hip.interpolator import film_conv
    _, fixture = load_golden("film_ops")
    x, w, b = FC.conv_case_inputs(name, cin, cout, k)
    n, h, wd = x.shape[0], x.shape[2], x.shape[3]
    cpad = cin if cin <= 8 else (cin + 7) // 8 * 8
    buf = ops.empty_image(n, cpad, h, wd, torch.float32, DEV)
    if cpad > cin:
        buf[:, cin:].zero_()
    ops.scale_into(_cl(x), out=buf[:, :cin])
    w, b = w.to(DEV), b.to(DEV)
    y = film_conv(buf, w, b)
    if act:
        y = ops.leaky_split(y, 0.2, out=y)[0]
    _check_conv(y, fixture[name], name)
    if k == 2:
        _check_conv(film_conv(buf, w, b, upsample2x=True), fixture[name + "_up"], name + "_up")
