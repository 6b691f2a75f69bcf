"""The kernels of csrc/small_ops.hip at their edges: the boundary transposes on every dtype pair around the 32 x 32 tile and with the
long axis past 65535 tiles, the second grid-stride sweep of the elementwise kernels (their grids stop at 8192 blocks: past 2 097 152
work items every thread loops), timestep_embedding beyond the two dims of its golden file, the thin-channel conv arms no other test
reaches, and the fused sampler steps at one element and past the grid cap.

Bounds.  Bitwise where the kernel performs exactly one rounding: the transposes (one round-to-nearest-even conversion, torch's), the
split_bf16 planes (hi = half(x); x - float(hi) is exact in fp32, lo = half of it).  Otherwise against an fp64 evaluation of the same
formula on the stored inputs:
  affine_cast, fp32 out : |got - ref| <= 2^-24 (|a x| + |ref|) - one rounding of the product, one of the sum (a fused multiply-add only
                          does better); where a x + b lies outside [lo, hi] by more than that, exactly lo / hi.
  affine_cast, half out : bitwise the fp32 result of the same call rounded once to the half type.  (A bound of the form |ref| 2^-9 HS,
                          as the fp32 one extended by "one half-type rounding", cannot hold for a correct kernel: bfloat16 keeps 8
                          significant bits, so rounding to nearest moves a value at the bottom of a binade by up to 2^-8 of itself -
                          1.00389 stores as 1.0 - and fp16 by 2^-11.  One rounding of the fp32 result is the stronger statement.)
  axpby_                : |got - ref| <= 2^-24 (|a x| + |b y| + |ref|), in the half type plus the output rounding |ref| 2^-8 HS (fp16: and
                          2^-25, half a step of its subnormals).
  silu, the convs       : check() of tests/test_hip_ops.py (silu runs on the hardware reciprocal and the fast exponential).
  timestep_embedding    : 2e-4 (one ulp of an argument near 1e3 rad, the existing test's bound), half output plus 2^-9 HS (|value| <= 1).
  split_mx              : the emulation and bounds of test_hip_ops.py::test_mx_planes_of_split_and_groupnorm.
  sampler steps         : the CPU fp32 chains and bounds of their own tests (test_hip_ops.py, test_inpaint_gpu.py, test_refiner_gpu.py).

The long axis (B2): nhwc_to_nchw of 1 x 3 x 1449 x 1449 puts 65 613 tiles of 32 pixels on grid.y (transpose_impl), an SDXL hires-fix decode
at 1536 x 1536 puts 73 728 there.  Measured on MI355X (ROCm 7.2): the device reports maxGridSize = (2147483647, 65536, 65536), yet the
runtime ACCEPTS the launch - an empty kernel launched with grid.y = 65 536, 65 613 and 73 728 returns hipSuccess and sees that gridDim.y -
and both transposes are bitwise right at this size, so the kernel stays as it is.  test_transposes_long_pixel_axis is the guard: a runtime
that starts to enforce the reported limit fails it, and the fix is then to carry both tile axes on grid.x.
The last test runs this file against the fp16 library in a child process.

Largest figure per test against its bound, measured on MI355X (`pytest -rP` prints every `[fig]` line):
                                                                 bf16 build                     fp16 build
  test_silu_sizes                                     rel-L2     1.56e-03 / 6.00e-03  (0.26)    2.00e-04 / 7.50e-04  (0.27)
  test_affine_cast_sizes                              err/bound  1.00e+00 / 1.00e+00  (1.00)    1.00e+00 / 1.00e+00  (1.00)
  test_axpby_sizes                                    err/bound  9.96e-01 / 1.00e+00  (1.00)    9.99e-01 / 1.00e+00  (1.00)
  test_split_mx_second_sweep                          hi8        5.72e-05 / 1.22e-04  (0.47)    5.72e-05 / 1.22e-04  (0.47)
  test_split_mx_second_sweep                          lo8        2.79e-08 / 5.96e-08  (0.47)    2.79e-08 / 5.96e-08  (0.47)
  test_timestep_embedding_dims_and_fractional_steps   half out   1.94e-03 / 2.15e-03  (0.90)    2.42e-04 / 4.44e-04  (0.54)
  test_timestep_embedding_dims_and_fractional_steps   fp32 out   3.54e-05 / 2.00e-04  (0.18)    3.54e-05 / 2.00e-04  (0.18)
  test_thin_conv_arms                                 rel-L2     2.26e-03 / 6.00e-03  (0.38)    2.82e-04 / 7.50e-04  (0.38)
  test_thin_conv_arms                                 max-abs    1.56e-02 / 7.01e-02  (0.22)    1.87e-03 / 8.03e-03  (0.23)
  test_cfg_euler_step_sizes / _ddim_ / _dpmpp2m_      max-abs    0 (bitwise the CPU chain at n = 1 and n = 2 097 409)
affine_cast and axpby_ reach their bounds and must: the bounds are the sums of the roundings the formula performs, each of which is attained
(half an ulp at the bottom of a binade) somewhere among two million elements.  The half-type timestep embedding sits at 0.90 because
2^-9 of its 2.15e-3 is the output rounding of values in [0.5, 1), also attained; its fp32 part is at 0.18.
"""
import math
import os
import re
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

from test_hip_ops import BF, DTYPES, HS, _dev, _mx_decode, check, fig, nhwc, q, rnd

pytestmark = pytest.mark.gpu

F32 = torch.float32
SWEEP = 8192 * 256          # work items one sweep of the capped grid covers
BIG = SWEEP + 257           # second sweep, ragged: one full block and one element more
SIZES = (1, 255, 257, BIG)
PAIRS = [(F32, F32), (F32, BF), (BF, F32), (BF, BF)]
PAIR_IDS = ["f32-f32", "f32-half", "half-f32", "half-half"]
HW_SHAPES = {1: (1, 1), 31: (1, 31), 33: (3, 11), 1000: (25, 40)}


def dev(t, dtype=None):
    t = t.to(_dev())
    return t.to(dtype) if dtype is not None else t


def is_channels_last(y):
    return y.permute(0, 2, 3, 1).is_contiguous()


# ------------------------------------------------------------------------------------------ B1: transposes around the tile
@pytest.mark.parametrize("sd,dd", PAIRS, ids=PAIR_IDS)
def test_transposes_around_the_tile(sd, dd):
    """N = 3, C x HW from {1, 31, 32, 33, 65} x {1, 31, 33, 1000}: below, at and past one 32 x 32 tile on either axis, both directions"""
    from cremage_amd import ops
    for C in (1, 31, 32, 33, 65):
        for hw, (H, W) in HW_SHAPES.items():
            x = rnd(3, C, H, W, seed=1000 + 7 * C + hw).to(sd)       # the stored source
            want = x.to(dd)                                           # one round-to-nearest-even conversion
            y = ops.nchw_to_nhwc(dev(x), dd)
            assert y.shape == x.shape and y.dtype == dd and is_channels_last(y), (C, hw, y.stride())
            assert torch.equal(y.cpu(), want), ("nchw_to_nhwc", C, hw)
            z = ops.nhwc_to_nchw(dev(x).contiguous(memory_format=torch.channels_last), dd)
            assert z.shape == x.shape and z.dtype == dd and z.is_contiguous(), (C, hw, z.stride())
            assert torch.equal(z.cpu(), want), ("nhwc_to_nchw", C, hw)


@pytest.mark.parametrize("sd,dd", PAIRS, ids=PAIR_IDS)
def test_concat_transpose_seam_inside_a_tile(sd, dd):
    """nchw2_to_nhwc == cat([a, b], 1) in channels-last: the a | b seam inside a tile, at a tile edge, b of one channel; (4, 5) at 64 x 64
    is the inpainting UNet's own boundary"""
    from cremage_amd import ops
    shapes = [(ca, cb, H, W) for ca, cb in ((4, 5), (31, 1), (33, 32), (4, 1)) for H, W in HW_SHAPES.values()] + [(4, 5, 64, 64)]
    for ca, cb, H, W in shapes:
        a, b = rnd(3, ca, H, W, seed=1100 + ca).to(sd), rnd(3, cb, H, W, seed=1200 + cb).to(sd)
        want = torch.cat([a, b], 1).to(dd)
        y = ops.nchw_to_nhwc(dev(a), dd, dev(b))
        assert y.shape == want.shape and y.dtype == dd and is_channels_last(y), (ca, cb, H, W, y.stride())
        assert torch.equal(y.cpu(), want), (ca, cb, H, W)


# ------------------------------------------------------------------------------------------ B2: the long axis
@pytest.mark.parametrize("sd", [F32, BF], ids=["f32", "half"])
def test_transposes_long_pixel_axis(sd):
    """1 x 3 x 1449 x 1449: 2 099 601 pixels, the first square past 65535 tiles of 32 (an SDXL hires-fix decode at 1536 x 1536 asks for
    73 728), to fp32, bitwise, both directions"""
    from cremage_amd import ops
    H = W = 1449
    assert H * W > 65535 * 32 >= (H - 1) * (W - 1)
    x = rnd(1, 3, H, W, seed=1300).to(sd)
    want = x.float()
    z = ops.nhwc_to_nchw(dev(x).contiguous(memory_format=torch.channels_last), F32)
    assert z.is_contiguous() and torch.equal(z.cpu(), want), "nhwc_to_nchw"
    y = ops.nchw_to_nhwc(dev(x), F32)
    assert is_channels_last(y) and torch.equal(y.cpu(), want), "nchw_to_nhwc"


# ------------------------------------------------------------------------------------------ B3: the second grid-stride sweep
def spread(n, seed):
    """N(0, 3^2) with the far tails of silu planted at both ends and around the sweep boundary"""
    x = rnd(n, seed=seed, scale=3.0)
    marks = torch.tensor([-100.0, -50.0, -20.0, 0.0, 20.0, 100.0])
    for at in (0, SWEEP - 3, n - 6):
        if 0 <= at and at + 6 <= n:
            x[at:at + 6] = marks
    if n == 1:
        x[0] = -100.0
    return x


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", SIZES)
def test_silu_sizes(dtype, n):
    from cremage_amd import ops
    x = spread(n, 1400 + n % 1000)
    got = ops.silu(dev(x, dtype))
    assert got.shape == (n,) and got.dtype == dtype
    check(got, F.silu(q(x, dtype).double()), dtype, f"silu n={n}")


def affine_bound(a, xs, ref):
    return 2.0 ** -24 * ((a * xs).abs() + ref.abs())


@pytest.mark.parametrize("sd", [F32, BF], ids=["f32", "half"])
@pytest.mark.parametrize("n", SIZES)
def test_affine_cast_sizes(sd, n):
    """to fp32: the derived bound; to the half type: one rounding of the fp32 result (see the module docstring)"""
    from cremage_amd import ops
    x = rnd(n, seed=1500 + n % 1000, scale=1.5)
    xd = dev(x, sd)
    xs = xd.cpu().double()
    for a, b, lo, hi in ((0.5, 0.5, 0.0, 1.0), (1.0 / 0.18215, -0.25, float("-inf"), float("inf"))):
        a32, b32 = torch.tensor(a, dtype=F32).double().item(), torch.tensor(b, dtype=F32).double().item()  # the kernel takes fp32 scalars
        raw = a32 * xs + b32
        ref = raw.clamp(lo, hi)
        got = ops.affine_cast(xd, a, b, F32, lo, hi)
        assert got.shape == (n,) and got.dtype == F32 and torch.isfinite(got).all()
        g = got.cpu().double()
        bound = affine_bound(a32, xs, ref)
        worst = ((g - ref).abs() / bound.clamp_min(1e-300)).max().item()
        fig(f"affine_cast n={n} a={a:.3g} err/bound", worst, 1.0)
        assert ((g - ref).abs() <= bound).all(), worst
        slack = affine_bound(a32, xs, raw)
        assert (g[raw > hi + slack] == hi).all() and (g[raw < lo - slack] == lo).all(), "clamped results must be exactly lo / hi"
        half = ops.affine_cast(xd, a, b, BF, lo, hi)
        assert half.dtype == BF and torch.equal(half, got.to(BF)), "half output is not the fp32 result rounded once"


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("n", SIZES)
def test_axpby_sizes(dtype, n):
    from cremage_amd import ops
    a, b = 0.25, 1.5
    x, y = dev(rnd(n, seed=1600 + n % 1000), dtype), dev(rnd(n, seed=1700 + n % 1000, scale=2.0), dtype)
    xs, ys = x.cpu().double(), y.cpu().double()
    ref = a * xs + b * ys
    out = ops.axpby_(y, x, a, b)
    assert out.data_ptr() == y.data_ptr() and torch.equal(x.cpu().double(), xs)
    bound = 2.0 ** -24 * ((a * xs).abs() + (b * ys).abs() + ref.abs())
    if dtype == BF:  # the output rounding: 8 significant bits (fp16: 11), and half a step of fp16's subnormals (2^-24) below 2^-14
        bound = bound + ref.abs() * 2.0 ** -8 * HS + (2.0 ** -25 if BF == torch.float16 else 0.0)
    err = (y.cpu().double() - ref).abs()
    worst = (err / bound.clamp_min(1e-300)).max().item()
    fig(f"axpby n={n} err/bound", worst, 1.0)
    assert (err <= bound).all(), worst


def channels_last_image(flat, c):
    """[pixels * c] values on the device as a [1, c, pixels, 1] channels-last image (no transpose launch: the storage is pixel-major)"""
    return flat.reshape(1, flat.numel() // c, 1, c).permute(0, 3, 1, 2)


def test_split_bf16_second_sweep():
    """n = 8 (8192 * 256 + 33) elements (67 MB): eight per thread, so the second sweep starts at element 16 777 216.  Magnitudes in
    [2^-3, 8], both signs; bitwise in both builds"""
    from cremage_amd import ops
    n = 8 * (SWEEP + 33)
    g = torch.Generator().manual_seed(1800)
    x = torch.exp2(torch.rand(n, generator=g) * 6.0 - 3.0) * (torch.randint(0, 2, (n,), generator=g) * 2 - 1).float()
    assert x.abs().min() >= 2.0 ** -3 and x.abs().max() <= 8.0
    hi, lo = ops.split_bf16(channels_last_image(dev(x), 8))
    assert hi.dtype == BF and lo.dtype == BF and is_channels_last(hi) and is_channels_last(lo) and tuple(hi.shape) == (1, 8, n // 8, 1)
    want_hi = x.to(BF)
    want_lo = (x - want_hi.float()).to(BF)
    assert torch.equal(hi.permute(0, 2, 3, 1).reshape(-1).cpu(), want_hi), "hi plane"
    assert torch.equal(lo.permute(0, 2, 3, 1).reshape(-1).cpu(), want_lo), "lo plane"


def test_split_mx_second_sweep():
    """C = 64 with 8192 * 256 / 8 + 5 pixels: eight channels per thread, 40 threads into the second sweep"""
    from cremage_amd import ops
    c, pixels = 64, SWEEP // 8 + 5
    x = rnd(pixels * c, seed=1900, scale=3.0)
    x[5 * c + 7] = 100.0                   # beyond the hi8 range: saturates at 28, must not wrap
    x[(pixels - 1) * c + 63] = -100.0      # and in the last thread of the second sweep
    x16, x8 = ops.split_mx(channels_last_image(dev(x), c))
    assert tuple(x16.shape) == (1, c, pixels, 1) and tuple(x8.shape) == (1, pixels, 1, 2 * c)
    h16 = x.to(torch.float16)
    assert torch.equal(x16.permute(0, 2, 3, 1).reshape(-1).cpu(), h16), "fp16 plane"
    hi, lo = _mx_decode(x8.cpu().reshape(pixels, 2 * c), c, *ops.MX_X_LOG2)
    xl, h16 = x.reshape(pixels, c), h16.float().reshape(pixels, c)
    sat = h16.clamp(-28.0, 28.0)
    e_hi = ((hi - sat).abs() - sat.abs() * 2.0 ** -4).max().item()
    e_lo = ((lo - (xl - h16)).abs() - (xl - h16).abs() * 2.0 ** -4).max().item()
    fig("split_mx hi8 error beyond 2^-4 |x|", e_hi, 2.0 ** -13)
    fig("split_mx lo8 error beyond 2^-4 |x - half(x)|", e_lo, 2.0 ** -24)
    assert e_hi <= 2.0 ** -13 and e_lo <= 2.0 ** -24
    assert hi[5, 7].item() == 28.0 and hi[pixels - 1, 63].item() == -28.0


# ------------------------------------------------------------------------------------------ B4: timestep_embedding
@pytest.mark.parametrize("dtype", DTYPES)
def test_timestep_embedding_dims_and_fractional_steps(dtype):
    """dim {2, 64, 65, 320, 321} (odd: a zero last column) x B {1, 3, 7} (B dim no multiple of the block) x t {0, 0.5, 1, 250.25, 999}
    against the formula in fp64 with the frequencies rounded to fp32 as the reference builds them"""
    from cremage_amd import ops
    steps = [0.0, 0.5, 1.0, 250.25, 999.0]
    bound = 2e-4 + (2.0 ** -9 * HS if dtype == BF else 0.0)
    worst = 0.0
    for dim in (2, 64, 65, 320, 321):
        half = dim // 2
        freqs = torch.exp(-math.log(10000) * torch.arange(start=0, end=half, dtype=F32) / half)
        for nb in (1, 3, 7):
            for start in range(len(steps)):
                t = torch.tensor([steps[(start + i) % len(steps)] for i in range(nb)])
                args = t.double()[:, None] * freqs.double()[None]
                ref = torch.cat([torch.cos(args), torch.sin(args), torch.zeros(nb, dim % 2, dtype=torch.float64)], -1)
                got = ops.timestep_embedding(dev(t), dim, dtype)
                assert tuple(got.shape) == (nb, dim) and got.dtype == dtype
                g = got.cpu().double()
                if dim % 2:
                    assert (g[:, -1] == 0).all(), (dim, nb)
                err = (g - ref).abs().max().item()
                assert err < bound, (dim, nb, t.tolist(), err)
                worst = max(worst, err)
    fig("timestep_embedding max-abs", worst, bound)


# ------------------------------------------------------------------------------------------ B5: thin-channel conv arms
IMAGES = [(9, 7), (1, 8), (5, 1), (3, 4)]   # 1 x 8: only the centre kernel row inside; 5 x 1: only the centre column; 3 x 4: both borders in one quad
CIN_KERNEL = [(8, 64, 3), (8, 64, 1), (9, 64, 1), (3, 64, 1), (4, 64, 1), (9, 64, 3)]  # thread = pixels x 8 output channels (W % 4: quad or not)
COUT_KERNEL = [(ci, co, ks) for ks in (1, 3) for ci, co in
               [(12, 3), (20, 5), (16, 4), (40, 8)] + [(ci, co) for ci in (12, 16) for co in (1, 2, 5, 6, 7)]]  # Cin % 8: the 8-wide or the scalar arm


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("ci,co,ks", CIN_KERNEL + COUT_KERNEL)
def test_thin_conv_arms(dtype, ci, co, ks):
    from cremage_amd import ops
    w, b = rnd(co, ci, ks, ks, seed=2000 + ci, scale=(ci * ks * ks) ** -0.5), rnd(co, seed=2001 + co)
    for H, W in IMAGES:
        x = rnd(2, ci, H, W, seed=2002 + H)
        ref = F.conv2d(q(x, dtype).double(), w.double(), b.double(), padding=ks // 2)
        got = ops.conv2d(nhwc(x, dtype), dev(w), dev(b), padding=ks // 2)
        assert is_channels_last(got) and got.dtype == dtype
        check(got, ref, dtype, f"conv_small {ci}->{co} k{ks} {H}x{W}")


# ------------------------------------------------------------------------------------------ B6: fused sampler steps
STEP_SIZES = (1, BIG)


@pytest.mark.parametrize("n", STEP_SIZES)
def test_cfg_euler_step_sizes(n):
    """the chain and bound of test_hip_ops.py::test_cfg_euler_step_matches_the_elementwise_chain, in fp32 on the CPU"""
    from cremage_amd import ops
    x, eps, noise = rnd(n, seed=2100), rnd(2 * n, seed=2101), rnd(n, seed=2102)
    sigma, dt, cfg, nscale = 3.7, -0.9, 7.5, 0.35
    for nz in (None, noise):
        e_u, e_c = eps[:n], eps[n:]
        den_u, den_c = x + e_u * (-sigma), x + e_c * (-sigma)
        den = den_u + cfg * (den_c - den_u)
        ref = x + ((x - den) / sigma) * dt
        if nz is not None:
            ref = ref + nz * nscale
        got = ops.cfg_euler_step_(dev(x), dev(eps), dev(nz) if nz is not None else None, sigma, dt, cfg, nscale)
        bound = 2e-6 * max(1.0, ref.abs().max().item())
        assert fig(f"cfg_euler_step n={n} max-abs", (got.cpu() - ref).abs().max().item(), bound) <= bound


@pytest.mark.parametrize("n", STEP_SIZES)
def test_cfg_ddim_step_sizes(n):
    """the chain and bound of test_inpaint_gpu.py::test_cfg_ddim_step_matches_elementwise_chain, with the sampler's own per-step scalars"""
    from cremage_amd import ops
    from cremage_amd.samplers import DDIMSampler, make_alphas_cumprod

    class M:
        num_timesteps = 1000
        alphas_cumprod = make_alphas_cumprod(1000)
        device = torch.device("cpu")
    x, eps, z = rnd(n, seed=2200), rnd(2 * n, seed=2201), rnd(n, seed=2202)
    for eta, cfg in ((0.0, 7.5), (1.0, 7.5), (1.0, 1.0)):
        s = DDIMSampler(M())
        s.make_schedule(20, ddim_eta=eta)
        for index in (19, 0):
            sq1ma, sqa, sqap, dirc, sig = s._step_scalars[index]
            eu, ec = eps[:n], eps[n:]
            e = eu + cfg * (ec - eu)
            x0 = (x - torch.tensor(sq1ma) * e) / torch.tensor(sqa)
            ref = torch.tensor(sqap) * x0 + torch.tensor(dirc) * e
            if sig != 0.0:
                ref = ref + torch.tensor(sig) * z
            got = dev(x)
            ops.cfg_ddim_step_(got, dev(eps), dev(z), cfg, sq1ma, sqa, sqap, dirc, sig)
            bound = 1e-6 * ref.abs().max().item()
            assert fig(f"cfg_ddim_step n={n} eta={eta} index={index} max-abs", (got.cpu() - ref).abs().max().item(), bound) <= bound


@pytest.mark.parametrize("n", STEP_SIZES)
def test_cfg_dpmpp2m_step_sizes(n):
    """the chain and bound of test_refiner_gpu.py::test_cfg_dpmpp2m_step_kernel: first, a middle and the last step of a 30-step schedule"""
    from cremage_amd import ops
    from cremage_amd.sgm_hip.sampling import LegacyDDPMDiscretization, dpmpp2m_multipliers
    sh = LegacyDDPMDiscretization()(30)
    mults = dpmpp2m_multipliers(sh)
    cfg = 5.0
    for i in (0, 14, len(mults) - 1):
        m1, m2, m3, m4, adv = mults[i]
        x, eps, old = rnd(n, seed=2300 + i) * float(sh[i]), rnd(2 * n, seed=2301 + i), rnd(n, seed=2302 + i)
        c_out = -float(sh[i])
        den_u, den_c = eps[:n] * c_out + x, eps[n:] * c_out + x
        den = den_u + cfg * (den_c - den_u)
        ref = m1 * x - m2 * (m3 * den - m4 * old) if adv else m1 * x - m2 * den
        xg, og = dev(x), dev(old)
        ops.cfg_dpmpp2m_step_(xg, dev(eps), og, c_out, cfg, m1, m2, m3 or 0.0, m4 or 0.0, adv)
        bx, bd = 1e-6 * ref.abs().max().item(), 1e-6 * den.abs().max().item()
        assert fig(f"cfg_dpmpp2m_step n={n} step {i} x max-abs", (xg.cpu() - ref).abs().max().item(), bx) <= bx
        assert fig(f"cfg_dpmpp2m_step n={n} step {i} denoised max-abs", (og.cpu() - den).abs().max().item(), bd) <= bd


N_TESTS = 4 + 4 + 2 + 3 * len(DTYPES) * len(SIZES) + 2 + len(DTYPES) + len(DTYPES) * len(CIN_KERNEL + COUT_KERNEL) + 3 * len(STEP_SIZES)
CHILD_TIME_LIMIT = 60  # seconds; measured on MI355X: the child takes 5.3 (interpreter and library start, then 1.8 for its 112 cases)


def test_this_file_against_the_fp16_library():
    """the same cases in ONE child process with CRG_HALF=f16 (the library is chosen when cremage_amd is imported; the pattern of
    tests/test_conv_subpixel.py).  In that child this test is deselected."""
    from tests.conftest import REPO
    from cremage_amd import _lib as L
    if L.HALF_F16:
        return  # this process already runs the fp16 library: the tests above were that run
    me = "tests/test_small_ops_gpu.py"
    cmd = [sys.executable, "-m", "pytest", me, "-m", "gpu", "-q", "-rs", "-p", "no:cacheprovider",
           "--deselect", me + "::test_this_file_against_the_fp16_library"]
    r = subprocess.run(cmd, cwd=REPO, env=dict(os.environ, CRG_HALF="f16"), capture_output=True, text=True, timeout=CHILD_TIME_LIMIT)
    tail = r.stdout[-6000:] + r.stderr[-3000:]
    assert r.returncode == 0, tail
    summary = [ln for ln in r.stdout.splitlines() if re.search(r"\b\d+ passed\b", ln)][-1]
    print(f"\n[parity] fp16 library, small kernels at their edges: {summary.strip()}")
    counts = {k: int(n) for n, k in re.findall(r"(\d+) (passed|failed|skipped|errors?|xfailed|xpassed|deselected)", summary)}
    assert counts == {"passed": N_TESTS, "deselected": 1}, (counts, tail)
