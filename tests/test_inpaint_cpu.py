"""SD1.5 inpainting, the parts that need no GPU: the YAML plug point, the 9-channel UNet's parameter contract against the reference's
inpainting UNet, the eta > 0 DDIM schedule, the hybrid DiffusionWrapper branch for a foreign module, the seed mapping and the host
glue of modules/sd/inpaint.py (make_batch_sd, padding to multiples of 64, blurred-mask compositing)."""
import hashlib
import os

import numpy as np
import pytest
import torch
import yaml

from tests.conftest import load_golden

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _inpaint_yaml():
    return yaml.safe_load(open(os.path.join(REPO, "cremage_amd", "configs", "v1-inpainting-hip.yaml")))["model"]["params"]


def test_inpainting_yaml_instantiates_hip_unet_with_nine_channels():
    from cremage_amd.ldm_hip.latent_diffusion import LatentInpaintDiffusion, instantiate_from_config
    from cremage_amd.ldm_hip.unet import UNetModel
    from cremage_amd.ldm_hip.vae import AutoencoderKL
    p = _inpaint_yaml()
    assert p["conditioning_key"] == "hybrid"
    assert p["unet_config"]["target"] == "cremage_amd.ldm_hip.unet.UNetModel"
    assert p["unet_config"]["params"]["in_channels"] == 9
    u = dict(p["unet_config"]["params"], model_channels=32, num_heads=4, context_dim=64)  # shrink: structure only
    unet = instantiate_from_config({"target": p["unet_config"]["target"], "params": u})
    assert isinstance(unet, UNetModel) and unet.in_channels == 9
    assert tuple(unet.input_blocks[0][0].weight.shape) == (32, 9, 3, 3)
    v = p["first_stage_config"]["params"]
    v = dict(v, ddconfig=dict(v["ddconfig"], ch=32))
    ldm = LatentInpaintDiffusion(unet, instantiate_from_config({"target": p["first_stage_config"]["target"], "params": v}),
                                 **{k: p[k] for k in ("linear_start", "linear_end", "timesteps", "scale_factor", "conditioning_key")})
    assert isinstance(ldm.first_stage_model, AutoencoderKL)
    assert ldm.model.conditioning_key == "hybrid" and ldm.concat_keys == ("mask", "masked_image")
    assert ldm.masked_image_key == "masked_image"


def test_inpaint_unet_state_dict_matches_reference_contract():
    """686 keys with the reference inpainting UNet's names and shapes (digest recorded from the reference's UNetModel(in_channels=9))."""
    from cremage_amd.ldm_hip.latent_diffusion import instantiate_from_config
    meta, _ = load_golden("inpaint_unet_sd15_full")
    with torch.device("meta"):
        unet = instantiate_from_config(_inpaint_yaml()["unet_config"])
    sd = unet.state_dict()
    items = sorted(f"{k}:{tuple(v.shape)}" for k, v in sd.items())
    assert len(items) == meta["n_keys"] == 686
    assert tuple(sd["input_blocks.0.0.weight"].shape) == tuple(meta["conv_in_shape"]) == (320, 9, 3, 3)
    assert hashlib.sha1("\n".join(items).encode()).hexdigest() == meta["keys_sha1"]


def test_ddim_eta_schedule_matches_reference():
    """make_schedule(eta=1): the sigma table of make_ddim_sampling_parameters (fp64 on the fp32 table values), stored in fp32."""
    from cremage_amd.samplers import DDIMSampler, make_alphas_cumprod
    meta, g = load_golden("traj_inpaint_ddim")

    class M:
        num_timesteps = 1000
        alphas_cumprod = make_alphas_cumprod(1000)
        device = torch.device("cpu")
    s = DDIMSampler(M())
    s.make_schedule(meta["S"], ddim_eta=meta["eta"])
    assert s.ddim_sigmas.dtype == torch.float32
    assert torch.equal(s.ddim_sigmas, g["ddim_sigmas"].to(torch.float32))
    assert all(v[4] > 0 for v in s._step_scalars)
    s.make_schedule(meta["S"], ddim_eta=0.0)
    assert not s.ddim_sigmas.any()


def test_hybrid_wrapper_concatenates_for_a_foreign_module():
    """DiffusionWrapper 'hybrid' hands any non-HIP module the reference's cat([x] + c_concat, dim 1) (ddpm.py:1520-1523)."""
    from cremage_amd.ldm_hip.latent_diffusion import DiffusionWrapper
    seen = {}

    class Probe(torch.nn.Module):
        def forward(self, x, t, context=None):
            seen.update(x=x, t=t, context=context)
            return x[:, :4]
    w = DiffusionWrapper(Probe(), "hybrid")
    x, m, z, ctx = torch.randn(2, 4, 8, 8), torch.randn(2, 1, 8, 8), torch.randn(2, 4, 8, 8), torch.randn(2, 77, 16)
    w(x, torch.tensor([1, 2]), c_concat=[m, z], c_crossattn=[ctx])
    assert torch.equal(seen["x"], torch.cat([x, m, z], 1)) and seen["context"] is ctx
    with pytest.raises(AssertionError):
        DiffusionWrapper(Probe(), "adm")


def test_seed_maps_to_numpy_start_code():
    from cremage_amd.pipeline import inpaint_start_code
    got = inpaint_start_code(1234, 2, 512, 384)
    ref = torch.from_numpy(np.random.RandomState(1234).randn(2, 4, 64, 48)).float()
    assert got.dtype == torch.float32 and torch.equal(got, ref)


def test_bbox_and_padding_to_multiples_of_64():
    from PIL import Image
    from cremage_amd import postprocess as PP
    assert PP.bbox_for_multiple_of_64(512, 512) == (512, 512)
    assert PP.bbox_for_multiple_of_64(63, 65) == (64, 128)
    assert PP.bbox_for_multiple_of_64(1, 640) == (64, 640)
    # landscape 100x50 into 128x64: the width fills, the height fits (64 rows) - no padding
    img = Image.new("RGB", (100, 50), (10, 200, 30))
    out, box = PP.resize_with_padding(img, 128, 64)
    assert out.size == (128, 64) and out.mode == "RGBA" and box == (0, 0, 128, 64)
    # 100x80 into 128x128: the resized height 102 fits, 26 rows of white padding split 13 / 13
    out, box = PP.resize_with_padding(Image.new("RGB", (100, 80), (10, 200, 30)), 128, 128)
    assert box == (0, 13, 128, 115)
    a = np.asarray(out)
    assert (a[:13] == 255).all() and (a[115:] == 255).all() and tuple(a[64, 64]) == (10, 200, 30, 255)
    # 61x100 into 128x128: the height fits (78 columns wide), the odd padding puts the extra column first
    out, box = PP.resize_with_padding(Image.new("RGB", (61, 100), (0, 0, 0)), 128, 128)
    assert box[1] == 0 and box[3] == 128 and box[2] - box[0] == int(61 * 128 / 100)
    assert box[0] == int((128 - 78) / 2) + (128 - 78) % 2


def test_make_batch_mask_threshold_and_masked_image():
    from PIL import Image
    from cremage_amd import postprocess as PP
    img = Image.fromarray(np.arange(4 * 4 * 3, dtype=np.uint8).reshape(4, 4, 3) * 5)
    m = np.zeros((4, 4, 3), dtype=np.uint8)
    m[0, :] = 255          # white: repaint
    m[1, :] = (127, 128, 128)  # luminance 127.6 -> "L" 128 -> 0.502 >= 0.5: repaint
    m[2, :] = (127, 127, 127)  # 0.498 < 0.5: keep
    image, mask, masked = PP.inpaint_batch(img, Image.fromarray(m))
    assert image.shape == (1, 3, 4, 4) and mask.shape == (1, 1, 4, 4) and masked.shape == (1, 3, 4, 4)
    assert torch.equal(image, torch.from_numpy(np.asarray(img).transpose(2, 0, 1)[None].astype(np.float32)) / 127.5 - 1.0)
    assert mask[0, 0, :, 0].tolist() == [1.0, 1.0, 0.0, 0.0]
    assert (masked[:, :, :2] == 0).all() and torch.equal(masked[:, :, 2:], image[:, :, 2:])


def test_gaussian_blur_11_matches_a_direct_2d_convolution():
    from cremage_amd import postprocess as PP
    rs = np.random.RandomState(3)
    a = (rs.rand(17, 23) > 0.6).astype(np.uint8) * 255
    got = PP.gaussian_blur_11(a)
    # direct 2-D form: sigma 2, reflect-101 border (index -1 -> 1)
    k = np.exp(-((np.arange(11) - 5.0) ** 2) / 8.0)
    k2 = np.outer(k, k) / k.sum() ** 2
    ref = np.zeros(a.shape)
    refl = lambda i, n: -i if i < 0 else (2 * (n - 1) - i if i >= n else i)  # noqa: E731
    for y in range(a.shape[0]):
        for x in range(a.shape[1]):
            ref[y, x] = sum(k2[i, j] * a[refl(y + i - 5, a.shape[0]), refl(x + j - 5, a.shape[1])] for i in range(11) for j in range(11))
    assert np.abs(got.astype(np.int64) - np.floor(ref + 0.5)).max() <= 1
    assert (PP.gaussian_blur_11(np.full((9, 9), 200, np.uint8)) == 200).all()


def test_composite_blends_inpainted_over_original_and_crops():
    from PIL import Image
    from cremage_amd import postprocess as PP
    orig = Image.new("RGBA", (64, 64), (10, 20, 30, 255))
    inp = Image.new("RGB", (64, 64), (250, 240, 230))
    black = Image.new("RGB", (64, 64), (0, 0, 0))
    white = Image.new("RGB", (64, 64), (255, 255, 255))
    assert (np.asarray(PP.composite_inpaint(orig, inp, black)) == (10, 20, 30)).all()
    assert (np.asarray(PP.composite_inpaint(orig, inp, white)) == (250, 240, 230)).all()
    m = np.zeros((64, 64, 3), np.uint8)
    m[:, 32:] = 255
    out = np.asarray(PP.composite_inpaint(orig, inp, Image.fromarray(m), bbox=(8, 4, 56, 60)))
    assert out.shape == (56, 48, 3)
    assert tuple(out[10, 0]) == (10, 20, 30) and tuple(out[10, -1]) == (250, 240, 230)
    row = out[10, :, 0].astype(int)
    assert (np.diff(row) >= 0).all() and 10 < row[24] < 250  # a soft edge around the mask boundary (x = 32 -> column 24)
