"""The gradient-domain ("poisson") paste on a real MI355X: ops.poisson_clone (crg_poisson_clone: a right-hand-side kernel and four batched
fp32 products on v_mfma_f32_32x32x2_f32) against the float64 host field of postprocess.poisson_clone_host, at the smallest shapes at
which the launches can go wrong - a 1 x 1 interior, an interior below one 32 x 32 MFMA tile with an odd K, one that is ragged across
the 32-wide wave tiles and the 64-wide block tiles in both dimensions, and one across 128 rows with K = 33 - and the face-fix chain
built on it against its host form.

The tolerance never comes from the code under test: tol = 8 x max|host fp32 field - host float64 field| of the case (the factor covers
another fp32 summation order in the MFMA chain and the multiplication by a rounded reciprocal where the host divides), and a case
whose tol reaches 0.02 fails, so that the tolerance cannot hide a wrong pixel.  CRG_TOL_REPORT=1 prints the measured errors."""
import os

import numpy as np
import pytest
import torch

from cremage_amd.synth import synth_input
from tests.test_hip_models import DEV

pytestmark = pytest.mark.gpu

REPORT = os.environ.get("CRG_TOL_REPORT") == "1"
PAD_Y, PAD_X = 9, 11  # the image is this much larger than the patch


def _content(kind, shape, seed):
    """uint8 [N, 3, rows, columns]: uniform noise (drives the field outside 0..255), or smooth waves with a little noise"""
    rng = np.random.RandomState(seed)
    if kind == "noise":
        return rng.randint(0, 256, shape).astype(np.uint8)
    yy, xx = np.mgrid[0:shape[2], 0:shape[3]]
    base = 120.0 + 90.0 * np.sin(xx / 7.0 + seed) * np.cos(yy / 5.0 + 0.3 * seed)
    return np.clip(base[None, None] + rng.normal(0.0, 3.0, shape) + 10.0 * np.arange(shape[1])[None, :, None, None], 0, 255).astype(np.uint8)


def _channels_last(t):
    t = t.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
    assert t.stride(1) == 1 and not t.is_contiguous()
    return t


def _host(img, pat, x, y, margin):
    """float64 fields [N, 3, n, m], and tol = 8 x the fp32 host arm's error against them"""
    from cremage_amd import postprocess as PP
    f64, f32 = [], []
    for i in range(img.shape[0]):
        a, p = np.ascontiguousarray(img[i].transpose(1, 2, 0)), np.ascontiguousarray(pat[i].transpose(1, 2, 0))
        f64.append(PP.poisson_clone_host(a, p, x, y, margin, return_field=True)[1].transpose(2, 0, 1))
        f32.append(PP.poisson_clone_host(a, p, x, y, margin, dtype=np.float32, return_field=True)[1].transpose(2, 0, 1))
    f64, f32 = np.stack(f64), np.stack(f32).astype(np.float64)
    return f64, 8.0 * np.abs(f32 - f64).max()


# (h, w), margin, where: "in" = offset (5, 3), "tl" = the image's top-left corner, "br" = its bottom-right corner
CASES = [((5, 5), 3, "in"), ((5, 5), 0, "in"), ((8, 21), 3, "tl"), ((8, 21), 1, "in"), ((41, 70), 3, "in"), ((41, 70), 3, "br"),
         ((134, 37), 3, "in")]


@pytest.mark.parametrize("kind", ["noise", "smooth"])
@pytest.mark.parametrize("hw,margin,where", CASES)
def test_poisson_clone_against_the_float64_field(hw, margin, where, kind):
    from cremage_amd import ops
    (h, w), N = hw, 2
    H, W = h + PAD_Y, w + PAD_X
    x, y = {"in": (5, 3), "tl": (0, 0), "br": (W - w, H - h)}[where]
    img = _content(kind, (N, 3, H, W), 10 + h)
    pat = _content(kind, (N, 3, h, w), 20 + w)
    u64, tol = _host(img, pat, x, y, margin)
    assert tol < 0.02, tol
    inside = np.zeros(img.shape, bool)
    inside[:, :, y + 2:y + h - 2, x + 2:x + w - 2] = True
    results = []
    # one image tensor contiguous (with a channels-last patch), one channels-last (with a contiguous patch)
    for layout in ("nchw", "channels_last"):
        image = torch.from_numpy(img).to(DEV)
        patch = torch.from_numpy(pat).to(DEV)
        if layout == "channels_last":
            image = _channels_last(image)
        else:
            patch = _channels_last(patch)
        strides = image.stride()
        field = torch.full((N, 3, h - 4, w - 4), float("nan"), device=DEV)
        got = ops.poisson_clone(image, patch, (x, y), margin, field_out=field)
        assert got is image and image.stride() == strides
        assert torch.equal(patch.cpu(), torch.from_numpy(pat))
        f = field.cpu().numpy().astype(np.float64)
        out = image.cpu().numpy()
        err = np.abs(f - u64).max()
        byte_err = np.abs(out[inside].astype(np.float64) - np.clip(u64, 0, 255).reshape(-1)).max()
        if REPORT:
            print(f"poisson {h}x{w} margin {margin} {where} {kind} {layout}: field range {u64.min():.1f}..{u64.max():.1f}, tol {tol:.3e}, "
                  f"|field_dev - u64| {err:.3e}, byte error {byte_err:.4f}")
        assert np.isfinite(f).all() and err <= tol, (err, tol)
        assert byte_err <= 0.5 + tol, (byte_err, tol)
        assert np.array_equal(out[~inside], img[~inside])
        assert np.array_equal(out[inside], np.clip(np.rint(f), 0, 255).astype(np.uint8).reshape(-1))  # the bytes are the stored field's
        # without field_out, on a clone: the same bytes
        again = torch.from_numpy(img).to(DEV)
        again = _channels_last(again) if layout == "channels_last" else again
        assert torch.equal(ops.poisson_clone(again, patch, (x, y), margin), image)
        results.append(image.cpu())
    assert torch.equal(results[0], results[1])  # the layout does not change a bit
    if margin == 3 and (h - 2 <= 6 or w - 2 <= 6):
        assert np.array_equal(results[0].numpy(), img)  # empty mask: the image comes back unchanged


def test_rejects_bad_arguments_before_any_launch():
    from cremage_amd import _lib as L
    from cremage_amd import ops
    img = torch.from_numpy(_content("noise", (2, 3, 40, 48), 1))
    pat = torch.from_numpy(_content("noise", (2, 3, 20, 24), 2))
    with pytest.raises(L.CrgError):
        ops.poisson_clone(img, pat, (3, 3))
    with pytest.raises(L.CrgError):
        ops.poisson_clone(img.to(DEV), pat, (3, 3))
    image, patch = img.to(DEV), pat.to(DEV)
    for bad in (lambda: ops.poisson_clone(image, patch, (25, 3)), lambda: ops.poisson_clone(image, patch, (3, 21)),
                lambda: ops.poisson_clone(image, patch, (-1, 3)), lambda: ops.poisson_clone(image, patch[:1], (3, 3)),
                lambda: ops.poisson_clone(image, patch[:, :2], (3, 3)), lambda: ops.poisson_clone(image.float(), patch, (3, 3)),
                lambda: ops.poisson_clone(image, patch, (3, 3), margin=-1),
                lambda: ops.poisson_clone(image, patch, (3, 3), field_out=torch.zeros((2, 3, 16, 21), device=DEV))):
        with pytest.raises(ValueError):
            bad()
    assert torch.equal(image.cpu(), img) and torch.equal(patch.cpu(), pat)  # nothing was written
    # no interior: nothing to do, nothing written
    assert ops.poisson_clone(image, patch[:, :, :4], (3, 3)) is image and torch.equal(image.cpu(), img)


# ------------------------------------------------------------------------------------------------ the face-fix chain
def _first_stage_img2img():
    """the tiny 8x first stage of tests/test_resample_gpu.py (DD8) as the "img2img": encode with a fixed noise, decode.  Bitwise
    deterministic, so the host and the device chain see the same faces as long as they hand it the same squares."""
    from cremage_amd import pipeline as P
    from tests.test_resample_gpu import _sd15_ldm
    ldm = _sd15_ldm()
    noise = synth_input("poisson.encnoise", (1, 4, 8, 8), 7).to(DEV)

    @torch.no_grad()
    def i2i(x):
        z = ldm.get_first_stage_encoding(ldm.encode_first_stage(x.to(DEV)), noise)
        return P.decode_images(ldm, z)
    return i2i


@pytest.mark.parametrize("faces", [[(40, 30, 50, 20)], [(25, 25, 20, 30), (110, 30, 14, 20)]], ids=["one_face", "two_faces"])
def test_face_fix_device_poisson_against_the_host_chain(faces):
    from PIL import Image
    from cremage_amd import postprocess as PP
    i2i = _first_stage_img2img()
    rng = np.random.RandomState(9)
    img = torch.from_numpy((rng.rand(3, 96, 160) * 1.2 - 0.1).astype(np.float32))
    plans = [PP.face_crop_plan(f, (160, 96), 64) for f in faces]
    if len(plans) == 2:  # the buffered crops do not overlap: the second face does not read what the first wrote
        assert plans[0].x + plans[0].w <= plans[1].x
    pil = PP.unit_tensor_to_pil(img)
    ref = np.asarray(PP.face_fix(pil, faces, i2i, 64, paste_mode="poisson"))
    # the host chain once more by hand, for the float64 field and the tolerance of every face
    near_half = np.zeros(ref.shape, bool)
    work = pil
    for plan in plans:
        face = PP.unpad_and_resize(PP.unit_tensor_to_pil(i2i(PP.pil_to_unit_tensor(PP.crop_and_pad(work, plan)))[0]), plan)
        a, p = np.asarray(work), np.asarray(face.convert("RGB"))
        out, u64 = PP.poisson_clone_host(a, p, plan.x, plan.y, return_field=True)
        u32 = PP.poisson_clone_host(a, p, plan.x, plan.y, dtype=np.float32, return_field=True)[1].astype(np.float64)
        tol = 8.0 * np.abs(u32 - u64).max()
        assert tol < 0.02, tol
        near_half[plan.y + 2:plan.y + plan.h - 2, plan.x + 2:plan.x + plan.w - 2] |= np.abs(u64 - np.floor(u64) - 0.5) <= tol
        work = Image.fromarray(out)
    assert np.array_equal(np.asarray(work), ref)
    got = PP.face_fix_device(img.to(DEV), faces, i2i, 64, paste_mode="poisson")
    assert got.dtype == torch.uint8 and got.is_cuda
    got = got.cpu().permute(1, 2, 0).numpy()
    diff = got.astype(np.int32) - ref.astype(np.int32)
    if REPORT:
        print(f"face_fix_device poisson, {len(faces)} face(s): {np.count_nonzero(diff)} of {diff.size} bytes differ, "
              f"{np.count_nonzero(near_half)} lie within tol of a half-integer")
    assert np.abs(diff).max() <= 1
    assert not (diff != 0)[~near_half].any()
    assert not np.array_equal(ref, np.asarray(pil))
    # the default mode still equals the host paste, to the bit
    plain = torch.from_numpy(np.array(PP.face_fix(pil, faces, i2i, 64))).permute(2, 0, 1)
    assert torch.equal(PP.face_fix_device(img.to(DEV), faces, i2i, 64).cpu(), plain)
    assert torch.equal(PP.face_fix_device(img.to(DEV), faces, i2i, 64, paste_mode="paste").cpu(), plain)


def test_txt2img_sdxl_facefix_poisson_paste():
    """BASELINE configuration 5's one-call form (the tiny chain of tests/test_hip_models.py) with paste_mode="poisson": the two passes are
    those of the default mode, the result is the host blend of their quantised images within one byte, and every pixel outside the
    boxes' inset-by-2 rectangles is the quantised first pass."""
    import torch.nn.functional as F
    from cremage_amd import pipeline as P
    from cremage_amd import postprocess as PP
    from tests.conftest import load_golden
    meta, _ = load_golden("traj_c5_chain")
    eng = P.build_synthetic_sdxl(meta["unet"], meta["dd"], DEV, unet_dtype=torch.float32, vae_dtype=torch.float32, seed=meta["seed"])
    B, L, seed = meta["B"], meta["L"], meta["seed"]
    c = {"crossattn": synth_input("c5.c", (B, 77, 128), seed).to(DEV), "vector": synth_input("c5.cv", (B, 96), seed).to(DEV)}
    uc = {"crossattn": synth_input("c5.uc", (B, 77, 128), seed).to(DEV), "vector": synth_input("c5.ucv", (B, 96), seed).to(DEV)}
    x0, en, fn = (synth_input(n, (B, 4, L, L), seed).to(DEV) for n in ("c5.x0", "c5.enc_noise", "c5.noise"))
    boxes = [tuple(b) for b in meta["boxes"]]
    assert all(sz >= 5 for _, _, sz in boxes)
    kw = dict(steps=meta["S2"], cfg_scale=meta["cfg"], height=2 * L, width=2 * L, fix_size=2 * L, strength=meta["strength"], x0=x0, enc_noise=en,
              fwd_noise=fn)
    plain, f1, f2 = P.txt2img_sdxl_facefix(eng, c, uc, boxes, **kw)
    out, g1, g2 = P.txt2img_sdxl_facefix(eng, c, uc, boxes, paste_mode="poisson", **kw)
    assert torch.equal(f1, g1) and torch.equal(f2, g2) and out.shape == plain.shape and out.dtype == plain.dtype
    quantise = lambda v: (np.float32(255.0) * v.float().clamp(0, 1).cpu().numpy()).astype(np.uint8)
    got = torch.round(out * 255.0).cpu().numpy()
    assert np.abs(got / np.float32(255.0) - out.cpu().numpy()).max() < 1e-6  # multiples of 1 / 255
    for i, (t, l, sz) in enumerate(boxes):
        base = quantise(f1[i]).transpose(1, 2, 0)
        face = quantise(F.interpolate(f2[i:i + 1], size=(sz, sz), mode="bilinear", align_corners=False)[0]).transpose(1, 2, 0)
        want = PP.poisson_clone_host(np.ascontiguousarray(base), np.ascontiguousarray(face), l, t).transpose(2, 0, 1)
        assert np.abs(got[i] - want).max() <= 1
        outside = np.ones(want.shape, bool)
        outside[:, t + 2:t + sz - 2, l + 2:l + sz - 2] = False
        assert np.array_equal(got[i][outside], base.transpose(2, 0, 1)[outside])
    assert not torch.equal(out, plain)
