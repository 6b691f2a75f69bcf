"""The device-side Lanczos resize on a real MI355X: ops.resample_u8 (crg_resample_u8) against PIL, byte for byte, at the smallest shapes
at which the kernel can go wrong - more than one 64 x 32 tile and ragged tiles, more than one 32-row source chunk per tile (ksize
far above 7), one pass only, a window with an offset, both source layouts and dtypes, both destination dtypes, fill and paste -
and the chains built on it (postprocess.face_fix_device, pipeline's `resample="device"`) against their host forms with torch.equal:
the package's UNet and VAE calls are bitwise deterministic, so any difference comes from the glue."""
import functools

import numpy as np
import pytest
import torch

from cremage_amd.synth import synth_input
from tests.conftest import load_golden
from tests.test_hip_models import DEV

pytestmark = pytest.mark.gpu

# 8x first stage (three down levels) for the pixel-space routes, as in tests/test_hires_routes_gpu.py
DD8 = dict(double_z=True, z_channels=4, resolution=64, in_channels=3, out_ch=3, ch=32, ch_mult=[1, 1, 2, 2], num_res_blocks=1,
           attn_resolutions=[], dropout=0.0)


def _unit(kind, shape, seed):
    """fp32 source content: random values (a few outside [0, 1]: the quantisation clamps), or binary 0 / 1 (the negative lobes clip)"""
    rng = np.random.RandomState(seed)
    if kind == "binary":
        return torch.from_numpy((rng.rand(*shape) > 0.5).astype(np.float32))
    return torch.from_numpy((rng.rand(*shape) * 1.2 - 0.1).astype(np.float32))


def _quantise(x: torch.Tensor) -> np.ndarray:
    """unit_tensor_to_pil's bytes: (255.0 * clamp(x, 0, 1)) in fp32, truncated"""
    return (np.float32(255.0) * x.clamp(0, 1).numpy()).astype(np.uint8)


def _pil_resize(u8_nchw: np.ndarray, H: int, W: int, window=None) -> torch.Tensor:
    """PIL's crop(window).resize((W, H), LANCZOS) of every image of an uint8 [N, 3, h, w] array -> uint8 [N, 3, H, W]"""
    from PIL import Image
    out = []
    for img in u8_nchw:
        pil = Image.fromarray(np.ascontiguousarray(img.transpose(1, 2, 0)))
        if window is not None:
            x0, y0, w, h = window
            pil = pil.crop((x0, y0, x0 + w, y0 + h))
        out.append(np.asarray(pil.resize((W, H), Image.LANCZOS)).transpose(2, 0, 1))
    return torch.from_numpy(np.stack(out))


@pytest.mark.parametrize("kind", ["random", "binary"])
@pytest.mark.parametrize("layout", ["nchw", "channels_last"])
def test_upscale_equals_pil(layout, kind):
    """batch 2, 3 channels, 40 x 56 -> 60 x 84 from fp32: two column tiles and two row tiles, both ragged"""
    from cremage_amd import ops
    x = _unit(kind, (2, 3, 40, 56), 1)
    ref = _pil_resize(_quantise(x), 60, 84)
    xd = x.to(DEV)
    if layout == "channels_last":
        xd = xd.permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
        assert xd.stride(1) == 1 and not xd.is_contiguous()
    keep = xd.clone()
    got = ops.resample_u8(xd, (60, 84), out_dtype=torch.uint8)
    assert got.dtype == torch.uint8 and torch.equal(got.cpu(), ref)
    assert torch.equal(xd, keep)
    # the fp32 store of the same bytes, and upscale_uint8's own result
    from cremage_amd import postprocess as PP
    assert torch.equal(ops.resample_u8(xd, (60, 84)).cpu(), ref.float() / 255.0)
    xc = xd.clamp(0, 1)  # upscale_uint8 takes images in [0, 1] (it does not clamp)
    assert torch.equal(PP.upscale_uint8_device(xc, 84, 60), PP.upscale_uint8(xc, 84, 60))


def test_window_offset_fill_and_affine_equal_crop_and_pad():
    """source 64 x 48, window (x 5, y 7, w 33, h 47) -> 50 x 71 at (3, 11) of a white 96 x 96 square in [-1, 1]: the host's crop_and_pad +
    pil_to_unit_tensor.  A kernel that clamps its taps to the image instead of the window differs along the window's edges."""
    from PIL import Image
    from cremage_amd import ops
    from cremage_amd import postprocess as PP
    x = _unit("random", (1, 3, 64, 48), 2)
    plan = PP.FaceCropPlan(5, 7, 33, 47, 50, 71, 3, 11, 96)
    pil = Image.fromarray(np.ascontiguousarray(_quantise(x)[0].transpose(1, 2, 0)))
    ref = PP.pil_to_unit_tensor(PP.crop_and_pad(pil, plan))
    out = torch.full((1, 3, 96, 96), float("nan"), device=DEV)
    got = ops.resample_u8(x.to(DEV), (71, 50), window=(5, 7, 33, 47), out=out, out_offset=(3, 11), out_affine=(2.0, -1.0), fill=1.0)
    assert got is out and torch.equal(got.cpu(), ref)
    assert torch.equal(PP.crop_and_pad_device(x.to(DEV), plan).cpu(), ref)
    # the same from the quantised uint8 image
    u8 = torch.from_numpy(_quantise(x)).to(DEV)
    assert torch.equal(PP.crop_and_pad_device(u8, plan).cpu(), ref)


@pytest.mark.parametrize("h,w,H,W", [(100, 75, 37, 29), (300, 8, 7, 8), (57, 31, 57, 62), (1, 9, 4, 9)])
@pytest.mark.parametrize("kind", ["random", "binary"])
def test_downscale_single_pass_and_odd_sizes_equal_pil(h, w, H, W, kind):
    """ksize 17 and 19 (100 x 75 -> 37 x 29, two row tiles, four source chunks), ksize 259 over ten source chunks (300 x 8 -> 7 x 8, vertical pass only), a
    horizontal pass only (57 x 31 -> 57 x 62) and a 1-row source; from uint8 and from fp32"""
    from cremage_amd import ops
    x = _unit(kind, (2, 3, h, w), 3)
    u8 = _quantise(x)
    ref = _pil_resize(u8, H, W)
    assert torch.equal(ops.resample_u8(torch.from_numpy(u8).to(DEV), (H, W), out_dtype=torch.uint8).cpu(), ref)
    assert torch.equal(ops.resample_u8(x.to(DEV), (H, W), out_dtype=torch.uint8).cpu(), ref)


def test_paste_without_fill_touches_nothing_outside():
    """uint8 destination 80 x 80 with a pattern, a 29 x 37 (w x h) result at (13, 9): PIL inside, every byte outside unchanged"""
    from cremage_amd import ops
    x = _unit("random", (2, 3, 50, 41), 4)
    ref = _pil_resize(_quantise(x), 37, 29)
    pattern = (torch.arange(2 * 3 * 80 * 80) % 251).to(torch.uint8).reshape(2, 3, 80, 80)
    out = pattern.to(DEV)
    got = ops.resample_u8(x.to(DEV), (37, 29), out=out, out_offset=(13, 9))
    assert got is out
    want = pattern.clone()
    want[:, :, 9:9 + 37, 13:13 + 29] = ref
    assert torch.equal(out.cpu(), want)


def test_fp32_store_of_every_byte():
    """v / 255.0 correctly rounded, then * 2.0 - 1.0 one rounding each: the CPU's values for all 256 bytes"""
    from cremage_amd import ops
    v = torch.arange(256, dtype=torch.uint8).reshape(1, 1, 16, 16)
    unit = v.float() / 255.0
    assert torch.equal(ops.resample_u8(v.to(DEV), (16, 16)).cpu(), unit)
    assert torch.equal(ops.resample_u8(v.to(DEV), (16, 16), out_affine=(2.0, -1.0)).cpu(), unit * 2.0 - 1.0)
    assert torch.equal(ops.resample_u8(v.to(DEV), (16, 16), out_dtype=torch.uint8).cpu(), v)


def test_resample_rejects_bad_arguments():
    from cremage_amd import _lib as L
    from cremage_amd import ops
    x = torch.zeros((1, 3, 16, 16), device=DEV)
    for kw, msg in ((dict(window=(4, 0, 16, 16)), "outside"), (dict(window=(0, 0, 0, 4)), "empty window"),
                    (dict(out=torch.zeros((1, 3, 8, 40), device=DEV)), "outside"), (dict(out=torch.zeros((1, 4, 32, 32), device=DEV)), "out of shape"),
                    (dict(out=torch.zeros((1, 3, 40, 40), device=DEV), out_offset=(9, 0)), "outside"), (dict(out_dtype=torch.float16), "out_dtype"),
                    (dict(out_dtype=torch.uint8, fill=300.0, out=torch.zeros((1, 3, 40, 40), device=DEV, dtype=torch.uint8)), "0..255")):
        with pytest.raises(L.CrgError, match=msg):
            ops.resample_u8(x, (32, 32), **kw)
    big = torch.zeros((1, 3, 32, 48), device=DEV)
    with pytest.raises(L.CrgError, match="overlap"):
        ops.resample_u8(big[:, :, :16, :16], (16, 32), out=big[:, :, 8:24, 16:48])
    with pytest.raises(L.CrgError, match="uint8 or float32"):
        ops.resample_u8(x.to(torch.bfloat16), (32, 32))


# ------------------------------------------------------------------------------------------------ chains
def _stand_in(x):
    """a deterministic "img2img": [1, 3, e, e] in [-1, 1] -> [0, 1], mirrored and inverted; one IEEE operation per step, so the CPU and the
    device give the same bits"""
    return 1.0 - ((x + 1.0) * 0.5).flip(-1)


def test_face_fix_device_equals_face_fix():
    """two overlapping faces on a 96 x 128 image - a landscape crop, then a portrait one clamped at the right border, which works on
    what the first left - against postprocess.face_fix on PIL images"""
    from cremage_amd import postprocess as PP
    img = _unit("random", (3, 96, 128), 5)
    faces = [(40, 30, 50, 20), (100, 40, 10, 30)]
    plans = [PP.face_crop_plan(f, (128, 96), 64) for f in faces]
    assert plans[0].w > plans[0].h and plans[1].h > plans[1].w and plans[1].x + plans[1].w == 128
    assert plans[1].x < plans[0].x + plans[0].w and plans[1].y < plans[0].y + plans[0].h
    ref = PP.face_fix(PP.unit_tensor_to_pil(img), faces, _stand_in, 64)
    ref = torch.from_numpy(np.array(ref)).permute(2, 0, 1)
    got = PP.face_fix_device(img.to(DEV), faces, _stand_in, 64)
    assert got.dtype == torch.uint8 and got.is_cuda and torch.equal(got.cpu(), ref)
    assert not torch.equal(ref, torch.from_numpy(_quantise(img)))


@functools.lru_cache(maxsize=None)
def _sd15_ldm():
    """the tiny SD1.5 LatentDiffusion of the fixtures (fp32-class nets) with the 8x first stage"""
    from cremage_amd import pipeline as P
    meta, _ = load_golden("traj_cn_ddim_img2img")
    return P.build_synthetic_ldm(meta["unet"], DD8, DEV, unet_dtype=torch.float32, vae_dtype=torch.float32, seed=meta["seed"])


@functools.lru_cache(maxsize=None)
def _control_ldm():
    from cremage_amd import pipeline as P
    meta, _ = load_golden("traj_cn_ddim_img2img")
    return P.build_synthetic_control_ldm(meta["unet"], DD8, DEV, unet_dtype=torch.float32, vae_dtype=torch.float32, seed=meta["seed"])


@functools.lru_cache(maxsize=None)
def _sdxl_engine():
    from cremage_amd import pipeline as P
    meta, _ = load_golden("traj_sdxl_hires_latent")
    return P.build_synthetic_sdxl(meta["unet"], DD8, DEV, unet_dtype=torch.float32, vae_dtype=torch.float32, seed=meta["seed"])


def _sdxl_case():
    meta, g = load_golden("traj_sdxl_hires_latent")
    B, seed = meta["B"], meta["seed"]
    ctx_c, ctx_uc = synth_input("xlhires.c", (B, 77, 128), seed), synth_input("xlhires.uc", (B, 77, 128), seed)
    c, uc = {"crossattn": ctx_c, "vector": g["cv"]}, {"crossattn": ctx_uc, "vector": g["ucv"]}
    c2, uc2 = {"crossattn": ctx_c, "vector": g["cv2"]}, {"crossattn": ctx_uc, "vector": g["ucv2"]}
    return meta, g, c, uc, c2, uc2


def _to_dev(d):
    return {k: v.to(DEV) for k, v in d.items()}


# faces of two 64 x 64 images: image 0 has two that overlap (portrait, then landscape clamped at the top), image 1 one
FACES = [[(30, 25, 6, 10), (28, 4, 14, 2)], [(22, 30, 12, 4)]]


def _both(fn):
    host, dev = fn("host"), fn("device")
    assert torch.isfinite(host).all() and host.is_cuda and dev.is_cuda and host.dtype == dev.dtype == torch.float32
    assert torch.equal(host, dev)
    return host


def test_face_fix_sdxl_device_equals_host():
    from cremage_amd import pipeline as P
    meta, g, c, uc, _, _ = _sdxl_case()
    eng, B, seed = _sdxl_engine(), meta["B"], meta["seed"]
    images = _unit("random", (B, 3, 64, 64), 6).clamp(0, 1).to(DEV)
    en, fn = (synth_input(n, (B, 4, 8, 8), seed).to(DEV) for n in ("rs.xl.encnoise", "rs.xl.fwdnoise"))
    out = _both(lambda r: P.face_fix_sdxl(eng, images, FACES, _to_dev(c), _to_dev(uc), steps=meta["S"], strength=0.5, cfg_scale=meta["cfg"],
                                          target_edge_len=64, enc_noise=en, fwd_noise=fn, resample=r))
    assert tuple(out.shape) == (B, 3, 64, 64) and not torch.equal(out, images)


def test_face_fix_sd15_device_equals_host():
    from cremage_amd import pipeline as P
    meta, _ = load_golden("traj_cn_ddim_img2img")
    ldm, B, seed = _sd15_ldm(), meta["B"], meta["seed"]
    c, uc = synth_input("cni2i.c", (B, 77, 96), seed).to(DEV), synth_input("cni2i.uc", (B, 77, 96), seed).to(DEV)
    images = _unit("random", (B, 3, 64, 64), 7).clamp(0, 1).to(DEV)
    en, fn = (synth_input(n, (B, 4, 8, 8), seed).to(DEV) for n in ("rs.sd.encnoise", "rs.sd.fwdnoise"))
    out = _both(lambda r: P.face_fix_sd15(ldm, images, FACES, c, uc, steps=meta["S"], strength=0.5, cfg_scale=meta["cfg"], target_edge_len=64,
                                          enc_noise=en, fwd_noise=fn, resample=r))
    assert tuple(out.shape) == (B, 3, 64, 64) and not torch.equal(out, images)
    # outside every crop rectangle the image is only quantised
    from cremage_amd import postprocess as PP
    plan = PP.face_crop_plan(FACES[1][0], (64, 64), 64)
    outside = torch.ones((3, 64, 64), dtype=torch.bool)
    outside[:, plan.y:plan.y + plan.h, plan.x:plan.x + plan.w] = False
    quantised = (torch.from_numpy(_quantise(images[1].cpu())).float() / 255.0 * 2.0 - 1.0 + 1.0) * 0.5
    assert torch.equal(out[1].cpu()[outside], quantised[outside])


@pytest.mark.parametrize("with_hint", [False, True])
def test_txt2img_hires_lanczos_device_equals_host(with_hint):
    """upscaler="lanczos" at the L of the existing hires tests, 64 x 64 -> 128 x 128; with a hint the default hint_hires is resized on
    the device as well"""
    from cremage_amd import pipeline as P
    meta, _ = load_golden("traj_cn_hires_latent")
    ldm = _control_ldm() if with_hint else _sd15_ldm()
    B, L, S, seed, f, cfg = meta["B"], meta["L"], meta["S"], meta["seed"], 2, meta["cfg"]
    c, uc = synth_input("cnhires.c", (B, 77, 96), seed).to(DEV), synth_input("cnhires.uc", (B, 77, 96), seed).to(DEV)
    x0 = synth_input("cnhires.x0", (B, 4, L, L), seed).to(DEV)
    hint = (synth_input("lz.hint", (B, 3, 8 * L, 8 * L), seed, 0.5).clamp(-1, 1) * 0.5 + 0.5).to(DEV) if with_hint else None
    enc_noise, fwd_noise = (synth_input(n, (B, 4, f * L, f * L), seed).to(DEV) for n in ("lz.encnoise", "lz.fwdnoise"))
    res = {r: P.txt2img_hires(ldm, c, uc, steps=S, sampler="DPM++ 2M", cfg_scale=cfg, height=8 * L, width=8 * L, x0=x0, factor=f, strength=0.5,
                              fwd_noise=fwd_noise, enc_noise=enc_noise, upscaler="lanczos", hint=hint, resample=r) for r in P.RESAMPLERS}
    for host, dev in zip(res["host"], res["device"]):
        assert torch.isfinite(host).all() and torch.equal(host, dev)
    assert tuple(res["device"][0].shape) == (B, 3, 8 * L * f, 8 * L * f)


def test_txt2img_sdxl_hires_lanczos_device_equals_host():
    from cremage_amd import pipeline as P
    meta, g, c, uc, c2, uc2 = _sdxl_case()
    c, uc, c2, uc2 = (_to_dev(d) for d in (c, uc, c2, uc2))
    eng, L, B, seed, f = _sdxl_engine(), meta["L"], meta["B"], meta["seed"], meta["factor"]
    L2 = int(L * f)
    enc_noise, fwd_noise = (synth_input(n, (B, 4, L2, L2), seed).to(DEV) for n in ("xllz.encnoise", "xllz.fwdnoise"))
    res = {r: P.txt2img_sdxl_hires(eng, c, uc, height=8 * L, width=8 * L, factor=f, strength=0.5, upscaler="lanczos", c_hires=c2, uc_hires=uc2,
                                   x0=g["x0"].to(DEV), fwd_noise=fwd_noise, enc_noise=enc_noise, steps=meta["S"], cfg_scale=meta["cfg"],
                                   resample=r) for r in P.RESAMPLERS}
    for host, dev in zip(res["host"], res["device"]):
        assert torch.isfinite(host).all() and torch.equal(host, dev)
    assert tuple(res["device"][0].shape) == (B, 3, 8 * L2, 8 * L2)
