"""Spot inpainting on a real MI355X: ops.blur_blend_u8 (crg_blur_blend_u8) against postprocess.blend_blurred_mask with torch.equal -
bit-equality is the criterion, no tolerance applies - and the device arms of the flows against their host arms on the tiny synthetic
LDMs of tests/test_resample_gpu.py: the package's UNet and VAE calls are bitwise deterministic, so any difference comes from the glue."""
import functools

import numpy as np
import pytest
import torch

from cremage_amd.synth import synth_input
from tests.conftest import load_golden
from tests.test_hip_models import DEV
from tests.test_resample_gpu import DD8

pytestmark = pytest.mark.gpu

TILE_W, TILE_H = 64, 32  # BB_TX x BB_TY of blur_blend.hip: one block's pixels
SIZES = [(6, 6), (7, 13), (64, 64), (100, 37), (TILE_H + 1, TILE_W + 1)]  # (H, W); 6 x 6 is the smallest a radius-5 reflect-101 accepts
MASKS = ["zeros", "full", "corners", "blobs", "grey"]


def _mask(kind, h, w, seed=0):
    rng = np.random.RandomState(seed)
    if kind == "zeros":
        return np.zeros((h, w), np.uint8)
    if kind == "full":
        return np.full((h, w), 255, np.uint8)
    if kind == "corners":
        m = np.zeros((h, w), np.uint8)
        m[0, 0] = m[0, -1] = m[-1, 0] = m[-1, -1] = 255
        return m
    if kind == "blobs":  # random binary blobs: a coarse random grid, upsampled
        coarse = rng.rand(-(-h // 5), -(-w // 5)) > 0.6
        return (np.kron(coarse, np.ones((5, 5)))[:h, :w] * 255).astype(np.uint8)
    return rng.randint(0, 256, (h, w)).astype(np.uint8)


def _images(h, w, c=3, seed=1, n=None):
    rng = np.random.RandomState(seed)
    shape = (h, w, c) if n is None else (n, h, w, c)
    return rng.randint(0, 256, shape).astype(np.uint8), rng.randint(0, 256, shape).astype(np.uint8)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _ref(orig, upd, grey):
    from cremage_amd import postprocess as PP
    return torch.from_numpy(PP.blend_blurred_mask(orig, upd, grey))


@pytest.mark.parametrize("kind", MASKS)
@pytest.mark.parametrize("h,w", SIZES)
def test_blur_blend_equals_host(h, w, kind):
    from cremage_amd import ops
    orig, upd = _images(h, w, seed=h * 131 + w)
    m = _mask(kind, h, w, seed=h + w)
    od, ud, md = _dev(orig), _dev(upd), _dev(m)
    got = ops.blur_blend_u8(od, ud, md)
    assert got.dtype == torch.uint8 and tuple(got.shape) == (h, w, 3)
    assert torch.equal(got.cpu(), _ref(orig, upd, m))
    assert torch.equal(od.cpu(), torch.from_numpy(orig)) and torch.equal(ud.cpu(), torch.from_numpy(upd))  # inputs are only read


@pytest.mark.parametrize("channels", [3, 4])
def test_rgb_and_rgba_masks_through_cv_gray(channels):
    """mask channels that differ, so the fixed-point weights matter; the alpha of an RGBA mask is ignored"""
    from cremage_amd import ops
    from cremage_amd import postprocess as PP
    h, w = 37, 70
    orig, upd = _images(h, w, seed=2)
    rgb = np.random.RandomState(3).randint(0, 256, (h, w, channels)).astype(np.uint8)
    rgb[5:20, 10:40, :3] = 255
    rgb[25:, :30, :3] = 0
    got = ops.blur_blend_u8(_dev(orig), _dev(upd), _dev(rgb), gray="cv_rgb")
    assert torch.equal(got.cpu(), _ref(orig, upd, PP._cv_gray(rgb)))
    # a one-channel mask with a trailing dimension of 1
    got1 = ops.blur_blend_u8(_dev(orig), _dev(upd), _dev(rgb[..., :1]))
    assert torch.equal(got1.cpu(), _ref(orig, upd, rgb[..., 0]))


def test_out_aliasing_original_and_given_out():
    from cremage_amd import ops
    h, w = 45, 71
    orig, upd = _images(h, w, seed=4)
    m = _mask("blobs", h, w, 5)
    ref = _ref(orig, upd, m)
    od = _dev(orig)
    got = ops.blur_blend_u8(od, _dev(upd), _dev(m), out=od)
    assert got is od and torch.equal(od.cpu(), ref)
    out = torch.full((h, w, 3), 7, dtype=torch.uint8, device=DEV)
    assert ops.blur_blend_u8(_dev(orig), _dev(upd), _dev(m), out=out) is out and torch.equal(out.cpu(), ref)


def test_strided_views_of_a_larger_rgba_image():
    """original / out: channels 0-2 of a 40 x 50 window of a 64 x 96 RGBA image, in place; the mask a window of a larger mask; all four
    channels of the same window as a second case.  Nothing outside the window, and no alpha byte in the first case, changes."""
    from cremage_amd import ops
    rng = np.random.RandomState(6)
    big = rng.randint(0, 256, (64, 96, 4)).astype(np.uint8)
    bigm = _mask("blobs", 64, 96, 7)
    y0, x0, h, w = 11, 23, 40, 50
    upd = rng.randint(0, 256, (h, w, 4)).astype(np.uint8)
    for ch in (3, 4):
        want = big.copy()
        want[y0:y0 + h, x0:x0 + w, :ch] = _ref(big[y0:y0 + h, x0:x0 + w, :ch], upd[..., :ch], bigm[y0:y0 + h, x0:x0 + w]).numpy()
        bd, md, ud = _dev(big), _dev(bigm), _dev(upd)
        view = bd[y0:y0 + h, x0:x0 + w, :ch]
        assert not view.is_contiguous()
        ops.blur_blend_u8(view, ud[..., :ch], md[y0:y0 + h, x0:x0 + w], out=view)
        assert torch.equal(bd.cpu(), torch.from_numpy(want))


def test_batch_of_two_with_own_and_shared_masks():
    from cremage_amd import ops
    h, w = 39, 67
    orig, upd = _images(h, w, seed=8, n=2)
    masks = np.stack([_mask("blobs", h, w, 9), _mask("grey", h, w, 10)])
    got = ops.blur_blend_u8(_dev(orig), _dev(upd), _dev(masks))
    assert torch.equal(got.cpu(), torch.stack([_ref(orig[i], upd[i], masks[i]) for i in range(2)]))
    shared = ops.blur_blend_u8(_dev(orig), _dev(upd), _dev(masks[0]))
    assert torch.equal(shared.cpu(), torch.stack([_ref(orig[i], upd[i], masks[0]) for i in range(2)]))


@pytest.mark.parametrize("inplace", [False, True])
def test_window_equals_full_image_run(inplace):
    """a blob in a 100 x 200 image (4 x 4 tiles): with window = the dilated bounding box most tiles skip the blur; the bytes are those
    of the full run, with a fresh destination (skipped tiles copy) and in place (skipped tiles do nothing)"""
    from cremage_amd import ops
    from cremage_amd import postprocess as PP
    h, w = 100, 200
    orig, upd = _images(h, w, seed=11)
    m = np.zeros((h, w), np.uint8)
    m[40:52, 90:131] = _mask("grey", 12, 41, 12) | 1
    window = PP.mask_window(m)
    assert window == (85, 35, 51, 22)
    od = _dev(orig)
    full = ops.blur_blend_u8(od, _dev(upd), _dev(m))
    got = ops.blur_blend_u8(od, _dev(upd), _dev(m), out=od if inplace else None, window=window)
    assert torch.equal(got.cpu(), full.cpu()) and torch.equal(full.cpu(), _ref(orig, upd, m))
    assert not torch.equal(full.cpu(), torch.from_numpy(orig))


def test_blur_blend_rejects_bad_arguments():
    from cremage_amd import _lib as L
    from cremage_amd import ops
    z = torch.zeros((16, 16, 3), dtype=torch.uint8, device=DEV)
    m = torch.zeros((16, 16), dtype=torch.uint8, device=DEV)
    with pytest.raises(L.CrgError):
        ops.blur_blend_u8(z.cpu(), z.cpu(), m.cpu())  # no CPU fallback
    with pytest.raises(L.CrgError, match="6x6"):
        ops.blur_blend_u8(z[:5], z[:5], m[:5])
    with pytest.raises(L.CrgError, match="does not fit"):
        ops.blur_blend_u8(z, z.clone(), m[:, :15])
    with pytest.raises(L.CrgError, match="does not fit"):
        ops.blur_blend_u8(z, z.clone(), m, gray="cv_rgb")
    with pytest.raises(L.CrgError, match="gray"):
        ops.blur_blend_u8(z, z.clone(), m, gray="luma")
    with pytest.raises(L.CrgError, match="uint8"):
        ops.blur_blend_u8(z.float(), z.float(), m)
    with pytest.raises(L.CrgError, match="outside"):
        ops.blur_blend_u8(z, z.clone(), m, window=(8, 0, 9, 4))
    base = torch.zeros((17, 16, 3), dtype=torch.uint8, device=DEV)
    with pytest.raises(L.CrgError, match="overlaps"):
        ops.blur_blend_u8(base[:16], z, m, out=base[1:])  # overlaps the original without being it
    upd = z.clone()
    with pytest.raises(L.CrgError, match="overlaps"):
        ops.blur_blend_u8(z, upd, m, out=upd)


# ------------------------------------------------------------------------------------------------ flows
def _stand_in(x):
    """a deterministic "img2img": [1, 3, e, e] in [-1, 1] -> [0, 1], mirrored and inverted; one IEEE operation per step"""
    return 1.0 - ((x + 1.0) * 0.5).flip(-1)


def _two_blob_mask():
    """96 x 128: a blob in the middle and one whose crop rectangle is clamped at the right and bottom borders"""
    m = np.zeros((96, 128), np.uint8)
    m[30:44, 40:60] = 255
    m[80:93, 110:125] = 200
    return m


def test_spot_fix_device_equals_spot_fix():
    from cremage_amd import postprocess as PP
    rng = np.random.RandomState(13)
    img = torch.from_numpy(rng.rand(3, 96, 128).astype(np.float32))
    m = _two_blob_mask()
    boxes = PP.mask_boxes(m)
    plans = [PP.face_crop_plan(b, (128, 96), 64) for b in boxes]
    assert len(boxes) == 2 and plans[0].x + plans[0].w == 128 and plans[0].y + plans[0].h == 96
    ref = torch.from_numpy(np.array(PP.spot_fix(PP.unit_tensor_to_pil(img), m, _stand_in, target_edge_len=64))).permute(2, 0, 1)
    got = PP.spot_fix_device(img.to(DEV), m, _stand_in, target_edge_len=64)
    assert got.dtype == torch.uint8 and got.is_cuda and tuple(got.shape) == (3, 96, 128) and torch.equal(got.cpu(), ref)
    quantised = (np.float32(255.0) * img.numpy()).astype(np.uint8)
    assert not torch.equal(ref, torch.from_numpy(quantised))
    blurred = PP.gaussian_blur_11(m)
    assert np.array_equal(got.cpu().numpy()[:, blurred == 0], quantised[:, blurred == 0])


@functools.lru_cache(maxsize=None)
def _sd15_ldm():
    from cremage_amd import pipeline as P
    meta, _ = load_golden("traj_cn_ddim_img2img")
    return P.build_synthetic_ldm(meta["unet"], DD8, DEV, unet_dtype=torch.float32, vae_dtype=torch.float32, seed=meta["seed"])


@functools.lru_cache(maxsize=None)
def _inpaint_ldm():
    """the tiny inpainting LatentDiffusion of the fixtures (9-channel UNet, fp32-class nets) with the 8x first stage"""
    from cremage_amd import pipeline as P
    meta, _ = load_golden("traj_inpaint_ddim")
    return P.build_synthetic_inpaint_ldm(meta["unet"], DD8, DEV, unet_dtype=torch.float32, vae_dtype=torch.float32, seed=meta["seed"])


def test_spot_fix_sd15_device_equals_host():
    from cremage_amd import pipeline as P
    meta, _ = load_golden("traj_cn_ddim_img2img")
    ldm, seed = _sd15_ldm(), meta["seed"]
    c, uc = synth_input("spot.c", (1, 77, 96), seed).to(DEV), synth_input("spot.uc", (1, 77, 96), seed).to(DEV)
    image = torch.from_numpy(np.random.RandomState(14).rand(3, 96, 128).astype(np.float32)).to(DEV)
    en, fn = (synth_input(n, (1, 4, 8, 8), seed).to(DEV) for n in ("spot.encnoise", "spot.fwdnoise"))
    m = _two_blob_mask()
    res = {r: P.spot_fix_sd15(ldm, image, m, c, uc, steps=meta["S"], strength=0.5, cfg_scale=meta["cfg"], resample=r, target_edge_len=64,
                              enc_noise=en, fwd_noise=fn) for r in P.RESAMPLERS}
    host, dev = res["host"], res["device"]
    assert torch.isfinite(host).all() and host.is_cuda and dev.is_cuda and host.dtype == dev.dtype == torch.float32
    assert tuple(host.shape) == (3, 96, 128) and torch.equal(host, dev)
    assert not torch.equal(host, image)


def _noise_sampler(shape, seed):
    calls = []

    def ns(sigma, index):
        calls.append(index)
        return synth_input(f"spot.noise{len(calls)}", shape, seed).to(DEV)
    return ns


def _u8_bytes(x):
    """[3, H, W] in [0, 1] (a u8 / 255 image) -> the bytes"""
    return (x * 255.0).round().to(torch.uint8)


@pytest.mark.parametrize("size", [(64, 64), (50, 40), (40, 50)])
def test_inpaint_image_device_equals_host(size):
    """width = height = 64: a 64 x 64 image goes in as it is; 50 x 40 and 40 x 50 (w x h) are resized and white-padded (both branches of
    resize_with_padding, the mask's padding white as well) and cropped at the end"""
    from PIL import Image
    from cremage_amd import pipeline as P
    meta, _ = load_golden("traj_inpaint_ddim")
    ldm, seed = _inpaint_ldm(), meta["seed"]
    c, uc = synth_input("spot.ic", (1, 77, 96), seed).to(DEV), synth_input("spot.iuc", (1, 77, 96), seed).to(DEV)
    w, h = size
    rng = np.random.RandomState(15)
    img = rng.randint(0, 256, (h, w, 3)).astype(np.uint8)
    m = np.zeros((h, w), np.uint8)
    m[h // 4:h // 2 + 6, w // 3:w // 3 + 14] = 255
    en = synth_input("spot.iencnoise", (1, 4, 8, 8), seed).to(DEV)
    kw = dict(width=64, height=64, steps=meta["S"], cfg_scale=meta["cfg"], eta=1.0, seed=seed, enc_noise=en)
    host = P.inpaint_image(ldm, Image.fromarray(img).convert("RGBA"), Image.fromarray(m), c, uc, glue="host",
                           noise_sampler=_noise_sampler((1, 4, 8, 8), seed), **kw)
    dev = P.inpaint_image(ldm, torch.from_numpy(img), torch.from_numpy(m), c, uc, glue="device",
                          noise_sampler=_noise_sampler((1, 4, 8, 8), seed), **kw)
    host = torch.from_numpy(np.array(host))
    assert dev.is_cuda and dev.dtype == torch.uint8 and tuple(dev.shape) == tuple(host.shape) and torch.equal(dev.cpu(), host)
    if size == (64, 64):
        from cremage_amd import postprocess as PP
        far = PP.gaussian_blur_11(m) == 0
        assert np.array_equal(host.numpy()[far], img[far]) and not np.array_equal(host.numpy(), img)
    else:
        assert tuple(host.shape) == ((51, 64, 3) if size == (50, 40) else (64, 51, 3))  # the crop scaled up: spot_inpaint's quirk


@pytest.mark.parametrize("hw", [(96, 128), (40, 50)])
def test_spot_inpaint_sd15_device_equals_host(hw):
    """max_edge_len 64: a 64 x 64 window of a 96 x 128 image (no padding), and a 40 x 50 image that is smaller than the window in
    both directions - the oversize patch, clipped at the image's border"""
    from cremage_amd import pipeline as P
    from cremage_amd import postprocess as PP
    meta, _ = load_golden("traj_inpaint_ddim")
    ldm, seed = _inpaint_ldm(), meta["seed"]
    c, uc = synth_input("spot.ic", (1, 77, 96), seed).to(DEV), synth_input("spot.iuc", (1, 77, 96), seed).to(DEV)
    H, W = hw
    image = torch.from_numpy(np.random.RandomState(16).randint(0, 256, (3, H, W)).astype(np.float32) / np.float32(255.0)).to(DEV)
    m = np.zeros((H, W), np.uint8)
    m[H // 2:H // 2 + 12, W // 2 + 3:W // 2 + 20] = 255
    m[H // 2 - 9:H // 2 - 4, W // 2 - 8:W // 2 - 2] = 255
    en = synth_input("spot.iencnoise", (1, 4, 8, 8), seed).to(DEV)
    res = {g: P.spot_inpaint_sd15(ldm, image, m, c, uc, max_edge_len=64, steps=meta["S"], cfg_scale=meta["cfg"], eta=1.0, seed=seed, glue=g,
                                  noise_sampler=_noise_sampler((1, 4, 8, 8), seed), enc_noise=en) for g in P.GLUES}
    host, dev = res["host"], res["device"]
    assert torch.isfinite(host).all() and host.is_cuda and dev.is_cuda and tuple(host.shape) == (3, H, W)
    assert torch.equal(host, dev) and not torch.equal(host, image)
    x, y, w, h = PP.spot_window(PP.mask_single_box(m), (W, H), 64)
    if hw == (96, 128):
        outside = torch.ones((H, W), dtype=torch.bool)
        outside[y:y + h, x:x + w] = False
        assert (w, h) == (64, 64) and torch.equal(_u8_bytes(host.cpu())[:, outside], _u8_bytes(image.cpu())[:, outside])
    else:
        assert (x, y, w, h) == (0, 0, W, H)
