"""txt2img / img2img drivers over the HIP UNet + VAE: the numeric core of the reference's call sites
`sd.txt2img.generate` / `sd.img2img.generate` -> `image_generator.generate`
(modules/sd/image_generator.py:569-1268), without the app shell (prompt parsing, CLIP, PNG metadata, UI
queues - all out of scope).  Conditioning arrives as tensors ([b, 77*n, 768]), exactly what
`model.get_learned_conditioning` hands to the sampler at image_generator.py:785-808.

Step structure reproduced (file:line of the reference):
  txt2img : sampler.sample(S, conditioning=c, batch_size, shape=[4,H/8,W/8], cfg, uc)      :958-967
            decode_first_stage per image, clamp((x+1)/2, 0, 1)                             :1007-1015
  img2img : encode_first_stage -> get_first_stage_encoding (posterior sample * 0.18215)    :721
            t_enc = int(strength * steps); DDIM stochastic_encode + decode                 :727, :147-248
  inpaint : modules/sd/inpaint.py:75-290 - mask + masked-image latents as c_concat (hybrid conditioning), start code from
            np.random.RandomState(seed), DDIM eta = 1 from x_T, decode                    :160-281
"""
from __future__ import annotations

import functools
from typing import Callable, Optional

import numpy as np
import torch

from . import ops
from .ldm_hip.latent_diffusion import LatentDiffusion, LatentInpaintDiffusion
from .ldm_hip.unet import UNetModel
from .ldm_hip.vae import AutoencoderKL
from . import samplers as K
from .samplers import DDIMSampler, EulerAncestralSampler, EulerSampler
from .synth import synth_fill_

SD15_UNET = dict(image_size=32, in_channels=4, out_channels=4, model_channels=320, attention_resolutions=[4, 2, 1],
                 num_res_blocks=2, channel_mult=[1, 2, 4, 4], num_heads=8, use_spatial_transformer=True, transformer_depth=1,
                 context_dim=768, use_checkpoint=True, legacy=False)  # v1-inference.yaml:29-44
SD15_VAE_DD = dict(double_z=True, z_channels=4, resolution=256, in_channels=3, out_ch=3, ch=128, ch_mult=[1, 2, 4, 4],
                   num_res_blocks=2, attn_resolutions=[], dropout=0.0)  # v1-inference.yaml:51-65

SAMPLERS = {"euler": EulerSampler, "euler_a": EulerAncestralSampler}  # sampler_utils.py:36-66 names "Euler", "Euler a"
# the rest of the menu: one table-driven class (samplers.KSampler), a constructor per key
SAMPLERS.update({key: functools.partial(K.KSampler, key=key) for key in K.K_SAMPLER_KEYS})


def _sampler(name: str):
    """(key, sampler constructor) of a SAMPLERS key or Cremage's menu name ("DPM++ 2M", ...)."""
    key = K.sampler_key(name)
    if key not in SAMPLERS:
        raise ValueError(f"sampler {name!r} is not a k-diffusion sampler (one of {sorted(SAMPLERS)}): DDIM runs through img2img / inpaint")
    return key, SAMPLERS[key]


def build_synthetic_ldm(unet_cfg=None, vae_dd=None, device="cuda", unet_dtype=torch.bfloat16, vae_dtype=torch.float32,
                        seed: int = 1234) -> LatentDiffusion:
    """LatentDiffusion with name-keyed synthetic weights (no checkpoint exists offline).
    Parameters are created on CPU in fp32, filled, then cast/moved - the same order as the reference's
    load_model_from_config (load_state_dict -> .half() -> .to(device), image_generator.py:345,489-493)."""
    unet = UNetModel(**(unet_cfg or SD15_UNET))
    vae = AutoencoderKL(vae_dd or SD15_VAE_DD, None, 4)
    synth_fill_(unet, seed, prefix="unet.")
    synth_fill_(vae, seed, prefix="vae.")
    ldm = LatentDiffusion(unet, vae)
    ldm.model.to(unet_dtype)
    ldm.first_stage_model.to(vae_dtype)
    return ldm.to(device).eval()


def build_synthetic_inpaint_ldm(unet_cfg=None, vae_dd=None, device="cuda", unet_dtype=torch.bfloat16, vae_dtype=torch.float32,
                                seed: int = 1234) -> LatentInpaintDiffusion:
    """LatentInpaintDiffusion (inpainting.yaml: hybrid conditioning, 9-channel UNet) with name-keyed synthetic weights."""
    unet = UNetModel(**dict(unet_cfg or SD15_UNET, in_channels=9))
    vae = AutoencoderKL(vae_dd or SD15_VAE_DD, None, 4)
    synth_fill_(unet, seed, prefix="unet.")
    synth_fill_(vae, seed, prefix="vae.")
    ldm = LatentInpaintDiffusion(unet, vae)
    ldm.model.to(unet_dtype)
    ldm.first_stage_model.to(vae_dtype)
    return ldm.to(device).eval()


def inpaint_start_code(seed: int, n: int, height: int, width: int) -> torch.Tensor:
    """The inpainting start latents of a Cremage seed (inpaint.py:166-169): np.random.RandomState(seed).randn(n, 4, H/8, W/8) as fp32."""
    return torch.from_numpy(np.random.RandomState(seed).randn(n, 4, height // 8, width // 8)).to(torch.float32)


def build_ldm_sharded(rank: int, device, unet_cfg=None, vae_dd=None, unet_dtype=torch.bfloat16, vae_dtype=torch.float32, seed: int = 1234):
    """The model of one rank of a batch-sharded run (bench.py --gpus N; tests/test_dist_cpu.py runs this very function under gloo):
    rank 0 materialises the synthetic weights, every other rank builds the same module tree UNINITIALISED in the same dtypes and
    receives parameters + buffers through ONE flat broadcast per (dtype, device) bucket (dist.broadcast_module_, whose header check
    makes every rank raise if the trees differ).  Returns (ldm, bytes broadcast)."""
    from . import dist as D
    if rank == 0:
        ldm = build_synthetic_ldm(unet_cfg, vae_dd, device=device, unet_dtype=unet_dtype, vae_dtype=vae_dtype, seed=seed)
    else:
        ldm = LatentDiffusion(UNetModel(**(unet_cfg or SD15_UNET)), AutoencoderKL(vae_dd or SD15_VAE_DD, None, 4))
        ldm.model.to(unet_dtype)
        ldm.first_stage_model.to(vae_dtype)
        ldm = ldm.to(device).eval()
    return ldm, D.broadcast_module_(ldm, src=0)


def build_synthetic_control_ldm(unet_cfg=None, vae_dd=None, device="cuda", unet_dtype=torch.bfloat16, vae_dtype=torch.float32, seed: int = 1234):
    """ControlLDM (cldm.py:345-393, cldm_v15.yaml) with name-keyed synthetic weights: ControlledUnetModel + ControlNet + VAE."""
    from .cldm_hip import ControlLDM, ControlledUnetModel, ControlNet
    cfg = unet_cfg or SD15_UNET
    unet = ControlledUnetModel(**cfg)
    cnet = ControlNet(hint_channels=3, **{k: v for k, v in cfg.items() if k != "out_channels"})
    vae = AutoencoderKL(vae_dd or SD15_VAE_DD, None, 4)
    synth_fill_(unet, seed, prefix="unet.")
    synth_fill_(cnet, seed, prefix="cn.")
    synth_fill_(vae, seed, prefix="vae.")
    ldm = ControlLDM(cnet, "hint", False, unet, vae)
    ldm.model.to(unet_dtype)
    ldm.control_model.to(unet_dtype)
    ldm.first_stage_model.to(vae_dtype)
    return ldm.to(device).eval()


@torch.no_grad()
def decode_images(ldm: LatentDiffusion, samples: torch.Tensor, batch_decode: bool = True) -> torch.Tensor:
    """latents [b,4,L,L] -> images [b,3,8L,8L] fp32 in [0,1] (image_generator.py:1007-1015).  The reference
    decodes one image at a time to fit 8-24 GB cards (`save_memory`, options.py:268-273); with 288 GB the
    whole batch is decoded in one pass unless `batch_decode=False`."""
    if batch_decode:
        x = ldm.decode_first_stage(samples)
    else:
        x = torch.cat([ldm.decode_first_stage(s[None]) for s in samples])
    return ops.affine_cast(x, 0.5, 0.5, torch.float32, 0.0, 1.0)


@torch.no_grad()
def trajectory_noise_sampler(steps: int, shape, device, generators=None) -> Callable:
    """Ancestral noise of a whole sampling run drawn UP FRONT - one randn per image generator (or one for the batch from the default
    generator) instead of one per image and step - and handed out step by step: the same number of Gaussian samples as the per-step
    `torch.randn_like(x)` of k-diffusion's default noise sampler (sampling.py:147-163), in 1 / b launches instead of `steps` / b * steps.
    The last step of a schedule that ends at sigma = 0 draws nothing, as in the reference."""
    if generators is not None:
        noise = torch.stack([torch.randn((steps,) + tuple(shape[1:]), generator=g, device=device) for g in generators], dim=1)
    else:
        noise = torch.randn((steps,) + tuple(shape), device=device)
    it = iter(range(steps))
    return lambda sigma, sigma_next: noise[next(it)]


@torch.no_grad()
def txt2img(ldm: LatentDiffusion, c: torch.Tensor, uc: Optional[torch.Tensor], *, steps: int = 20, sampler: str = "euler_a",
            cfg_scale: float = 7.5, height: int = 512, width: int = 512, x0: Optional[torch.Tensor] = None,
            noise_sampler: Optional[Callable] = None, decode: bool = True, hint: Optional[torch.Tensor] = None, generators=None):
    """Returns (images or None, final latents).  `hint` ([b,3,H,W] in [0,1], ControlLDM only): the ControlNet control image;
    conditioning becomes {"c_crossattn": [c], "c_concat": [hint]} for both the positive and the negative prompt
    (image_generator.py:795-808).  `generators`: one torch.Generator per image (seed + global image index, cremage_amd.dist.image_seed):
    the initial latents (unless x0 is given) and the ancestral noise of image i come from generators[i], so that a batch sharded over
    GPUs draws what the unsharded batch draws.  Without an explicit `noise_sampler` the ancestral sampler's noise is drawn once per run
    (trajectory_noise_sampler).  `sampler`: a SAMPLERS key or Cremage's menu name; the table-driven samplers that draw noise get a
    trajectory_noise_sampler sized by their plan's draw count, DPM++ SDE a samplers.BrownianPairNoise (per image with `generators`)."""
    b = c.shape[0]
    dev = c.device
    sampler, make = _sampler(sampler)
    if x0 is None and generators is not None:
        x0 = torch.stack([torch.randn((4, height // 8, width // 8), generator=g, device=dev) for g in generators])
    if noise_sampler is None and sampler == "euler_a" and dev.type == "cuda":
        noise_sampler = trajectory_noise_sampler(steps, (b, 4, height // 8, width // 8), dev, generators)
    if hint is not None:
        c = {"c_crossattn": [c], "c_concat": [hint]}
        uc = {"c_crossattn": [uc], "c_concat": [hint]} if uc is not None else None
    shape = [4, height // 8, width // 8]
    smp = make(ldm)
    if noise_sampler is None and sampler in K.K_SAMPLER_KEYS and dev.type == "cuda":
        if sampler == "dpmpp_sde":
            noise_sampler = K.BrownianPairNoise((b, *shape), dev, generators=generators)
        else:
            draws = K.plan_draws(smp.plan(steps))
            noise_sampler = trajectory_noise_sampler(draws, (b, *shape), dev, generators) if draws else None
    smp.noise_sampler = noise_sampler
    samples, _ = smp.sample(S=steps, conditioning=c, batch_size=b, shape=shape, verbose=False,
                            unconditional_guidance_scale=cfg_scale, unconditional_conditioning=uc, x0=x0)
    return (decode_images(ldm, samples) if decode else None), samples


UPSCALERS = ("latent", "lanczos")  # Cremage's hires-fix upscalers (opt.hires_fix_upscaler), lower-cased


def _upscaler(name: str) -> str:
    key = str(name).lower()
    if key not in UPSCALERS:
        raise ValueError(f"unknown hires-fix upscaler {name!r} (one of {list(UPSCALERS)})")
    return key


RESAMPLERS = ("host", "device")  # where the pixel-space Lanczos glue runs: PIL on the host, or ops.resample_u8


def _resampler(name: str) -> str:
    if name not in RESAMPLERS:
        raise ValueError(f"unknown resample {name!r} (one of {list(RESAMPLERS)})")
    return name


def _lanczos_scaled(PP, images: torch.Tensor, width: int, height: int, resample: str, signed: bool) -> torch.Tensor:
    """postprocess.upscale_uint8 on the host or on the device; `signed`: * 2 - 1 behind it (folded into the device store)."""
    if resample == "device":
        return PP.upscale_uint8_device(images, width, height, (2.0, -1.0) if signed else (1.0, 0.0))
    up = PP.upscale_uint8(images, width, height).contiguous()
    return up * 2.0 - 1.0 if signed else up


def _control_cond(c, uc, hint):
    """The two dict conditionings of a ControlNet run, holding the SAME hint object (image_generator.py:839-846, guess_mode False), so
    that the doubled c_concat gets the CFG mark (samplers.cat_cond_dict)."""
    return {"c_crossattn": [c], "c_concat": [hint]}, ({"c_crossattn": [uc], "c_concat": [hint]} if uc is not None else None)


def upscale_encode_latents(smp, base: torch.Tensor, factor: float, t_enc: int, steps: int, fwd_noise: Optional[torch.Tensor] = None,
                           fused: Optional[bool] = None) -> torch.Tensor:
    """The latent upscaler's F.interpolate(bilinear) + k-diffusion stochastic_encode (image_generator.py:894, :975 and
    k_diffusion_samplers.py:255-296).  `fused` (None: fp32 device latents): ONE launch, ops.upscale_noise with the host-computed
    sqrt(acp_t) and sqrt(1 - acp_t) of smp.encode_scalars; otherwise the two torch calls.  The noise is `fwd_noise`, or randn of
    the upscaled shape."""
    import torch.nn.functional as F
    b = base.shape[0]
    if fused is None:
        fused = base.is_cuda and base.dtype == torch.float32
    if not fused:
        up = F.interpolate(base, scale_factor=factor, mode="bilinear", align_corners=False)
        return smp.stochastic_encode(up, torch.tensor([t_enc] * b, device=up.device), sampling_steps=steps, noise=fwd_noise)
    if fwd_noise is None:
        fwd_noise = torch.randn((b, base.shape[1], ops.upscaled_size(base.shape[2], factor), ops.upscaled_size(base.shape[3], factor)),
                                device=base.device)
    a, s = smp.encode_scalars(t_enc, steps)
    return ops.upscale_noise(base.contiguous(), factor, fwd_noise.contiguous(), a, s, 1.0)


@torch.no_grad()
def txt2img_hires(ldm: LatentDiffusion, c: torch.Tensor, uc: Optional[torch.Tensor], *, steps: int = 20, sampler: str = "euler_a",
                  cfg_scale: float = 7.5, height: int = 512, width: int = 512, factor: float = 2.0, strength: float = 0.5,
                  x0: Optional[torch.Tensor] = None, fwd_noise: Optional[torch.Tensor] = None, noise_sampler: Optional[Callable] = None,
                  decode: bool = True, upscaler: str = "latent", hint: Optional[torch.Tensor] = None,
                  hint_hires: Optional[torch.Tensor] = None, enc_noise: Optional[torch.Tensor] = None, resample: str = "host"):
    """Hires-fix (image_generator.py:889-932, :958-999, :1020-1098): txt2img at (height, width), an upscale by `factor`, forward
    diffusion to t_enc = int(strength * steps) (k_diffusion_samplers.py:255-296) and a denoise of the last t_enc + 1 sigmas at the
    larger size (img2img_sampling :192-211, :227-246).  `sampler`: a SAMPLERS key or Cremage's menu name, used by both passes.
    `upscaler`:
      "latent"  - bilinear F.interpolate of the final latents.  On a ControlNet run (`hint`) with fp32 device latents the upscale and
                  the forward diffusion are ONE launch (ops.upscale_noise).  Without `hint` the two torch calls stay: the launch rounds
                  every operation once, ATen's device kernel contracts its blend into fused multiply-adds, so the results differ in
                  the last bits and the existing fixtures of this route keep the arithmetic they were recorded against.
      "lanczos" - decode, postprocess.upscale_uint8 (an APPROXIMATION of the reference's cv2.INTER_LANCZOS4, see there), * 2 - 1,
                  encode (`enc_noise`: the posterior sample's noise), forward diffusion, second pass.
    `hint` ([b,3,height,width] in [0,1], ControlLDM only): both passes run dict conditioning; the second pass uses `hint_hires`
    ([b,3,height*factor,width*factor]), by default postprocess.upscale_uint8(hint) - the same approximation, of scale_control_image
    (:552-562).  The ControlNet's one-entry hint cache then holds the second pass' guided hint.  Returns (images, latents, base
    latents).
    `resample` ("host", the default, or "device"): where upscale_uint8 runs with upscaler "lanczos" - the upscaler's own and the default
    hint_hires'; the "latent" route is not changed by it.  "device" is postprocess.upscale_uint8_device: one launch, no transfer and no synchronisation between the passes, the
    same tensors to the bit."""
    from . import postprocess as PP
    upscaler = _upscaler(upscaler)
    resample = _resampler(resample)
    b = c.shape[0]
    smp = _sampler(sampler)[1](ldm)
    smp.noise_sampler = noise_sampler
    cond, ucond = _control_cond(c, uc, hint) if hint is not None else (c, uc)
    base, _ = smp.sample(S=steps, conditioning=cond, batch_size=b, shape=[4, height // 8, width // 8], verbose=False,
                         unconditional_guidance_scale=cfg_scale, unconditional_conditioning=ucond, x0=x0)
    t_enc = int(strength * steps)
    big_w, big_h = int(width * factor), int(height * factor)
    if upscaler == "latent":
        z_enc = upscale_encode_latents(smp, base, factor, t_enc, steps, fwd_noise, fused=None if hint is not None else False)
    else:
        scaled = _lanczos_scaled(PP, decode_images(ldm, base), big_w, big_h, resample, True)
        init_latent = ldm.get_first_stage_encoding(ldm.encode_first_stage(scaled), enc_noise)
        z_enc = smp.stochastic_encode(init_latent, torch.tensor([t_enc] * b, device=init_latent.device), sampling_steps=steps,
                                      noise=fwd_noise)
    if hint is not None:
        if hint_hires is None:
            hint_hires = _lanczos_scaled(PP, hint, big_w, big_h, resample if upscaler == "lanczos" else "host", False)
        cond, ucond = _control_cond(c, uc, hint_hires)
    samples, _ = smp.sample(S=steps, conditioning=cond, batch_size=b, shape=list(z_enc.shape[1:]), verbose=False,
                            unconditional_guidance_scale=cfg_scale, unconditional_conditioning=ucond, x0=z_enc, denoising_steps=t_enc)
    return (decode_images(ldm, samples) if decode else None), samples, base


@torch.no_grad()
def img2img(ldm: LatentDiffusion, init_image: torch.Tensor, c: torch.Tensor, uc: Optional[torch.Tensor], *, steps: int = 20,
            strength: float = 0.75, cfg_scale: float = 7.5, enc_noise: Optional[torch.Tensor] = None,
            fwd_noise: Optional[torch.Tensor] = None, decode: bool = True, hint: Optional[torch.Tensor] = None):
    """SD1.5 img2img as the reference drives it: sampler forced to DDIM (image_generator.py:679-681).  `hint` ([b,3,H,W] in [0,1],
    ControlLDM only): ControlNet img2img (:850-875, img2img_sampling :168-190) - the two dict conditionings hold the same hint object
    as txt2img builds them, and DDIMSampler.decode runs them through its fused step."""
    b = init_image.shape[0]
    init_latent = ldm.get_first_stage_encoding(ldm.encode_first_stage(init_image), enc_noise)
    t_enc = int(strength * steps)
    smp = DDIMSampler(ldm)
    smp.make_schedule(ddim_num_steps=steps, ddim_eta=0.0, verbose=False)
    z_enc = smp.stochastic_encode(init_latent, torch.tensor([t_enc] * b, device=init_latent.device), noise=fwd_noise)
    if hint is not None:
        c, uc = _control_cond(c, uc, hint)
    samples = smp.decode(z_enc, c, t_enc, unconditional_guidance_scale=cfg_scale, unconditional_conditioning=uc)
    return (decode_images(ldm, samples) if decode else None), samples


@torch.no_grad()
def inpaint(ldm: LatentDiffusion, image, mask, c: torch.Tensor, uc: Optional[torch.Tensor], *, steps: int = 50, cfg_scale: float = 7.5,
            eta: float = 1.0, seed: Optional[int] = None, noise_sampler: Optional[Callable] = None, enc_noise: Optional[torch.Tensor] = None,
            decode: bool = True):
    """SD1.5 inpainting as modules/sd/inpaint.py:75-290 drives it, on an inpainting LatentDiffusion (9-channel UNet, hybrid conditioning).

    image [n, 3, H, W] in [-1, 1] and mask [n, 1, H, W] (white = repaint; thresholded at 0.5) on the model's device, H and W multiples of
    64 (postprocess.inpaint_batch builds both from PIL images as make_batch_sd does, postprocess.resize_with_padding pads to 64).
    c_concat = cat([mask nearest-downsampled to H/8 x W/8, get_first_stage_encoding(encode(image * (mask < 0.5)))]) (:218-227) - one
    tensor in both the conditional and the unconditional dict (:244-245), so the HIP UNet may share its CFG prefix; start code from
    np.random.RandomState(seed) (:166-169; torch.randn when seed is None); DDIM with eta (1.0 in the reference) from that start code;
    decode and clamp((x + 1) / 2, 0, 1).  `enc_noise`: the posterior sample's noise; `noise_sampler(sigma, index)`: DDIM's per-step z.
    Returns (images [n, 3, H, W] in [0, 1] or None, final latents)."""
    import torch.nn.functional as F
    n = image.shape[0]
    dev = ldm.device
    image = image.to(dev, torch.float32)
    m = (mask.to(dev, torch.float32) >= 0.5).to(torch.float32)
    masked = image * (m < 0.5)
    z_masked = ldm.get_first_stage_encoding(ldm.encode_first_stage(masked), enc_noise).to(torch.float32)
    hl, wl = z_masked.shape[-2:]  # H/8 x W/8 with the SD VAE
    m_lat = F.interpolate(m, size=(hl, wl))  # nearest, the reference's default mode
    c_cat = torch.cat([m_lat, z_masked], dim=1)
    cond = {"c_concat": [c_cat], "c_crossattn": [c]}
    uc_full = {"c_concat": [c_cat], "c_crossattn": [uc]} if uc is not None else None
    x_T = inpaint_start_code(seed, n, 8 * hl, 8 * wl).to(dev) if seed is not None else torch.randn((n, 4, hl, wl), device=dev)
    smp = DDIMSampler(ldm)
    samples, _ = smp.sample(steps, n, [4, hl, wl], cond, eta=eta, x_T=x_T, unconditional_guidance_scale=cfg_scale,
                            unconditional_conditioning=uc_full, noise_sampler=noise_sampler)
    return (decode_images(ldm, samples) if decode else None), samples


# ---------------------------------------------------------------------------------------------- SDXL (config 3)
SDXL_UNET = dict(adm_in_channels=2816, num_classes="sequential", use_checkpoint=True, in_channels=4, out_channels=4,
                 model_channels=320, attention_resolutions=[4, 2], num_res_blocks=2, channel_mult=[1, 2, 4], num_head_channels=64,
                 use_linear_in_transformer=True, transformer_depth=[1, 2, 10], context_dim=2048,
                 spatial_transformer_attn_type="softmax-xformers")  # sd_xl_base.yaml:17-33
SDXL_VAE_DD = dict(SD15_VAE_DD, attn_type="vanilla-xformers")       # sd_xl_base.yaml:80-92
SDXL_REFINER_UNET = dict(adm_in_channels=2560, num_classes="sequential", use_checkpoint=True, in_channels=4, out_channels=4,
                         model_channels=384, attention_resolutions=[4, 2], num_res_blocks=2, channel_mult=[1, 2, 4, 4], num_head_channels=64,
                         use_linear_in_transformer=True, transformer_depth=4, context_dim=[1280, 1280, 1280, 1280],
                         spatial_transformer_attn_type="softmax-xformers")  # sd_xl_refiner.yaml:17-33


def build_synthetic_sdxl(unet_cfg=None, vae_dd=None, device="cuda", unet_dtype=torch.bfloat16, vae_dtype=torch.float32, seed: int = 1234,
                         fill: bool = True):
    """DiffusionEngine-like container with name-keyed synthetic weights (UNet fp16/bf16, VAE fp32 as the reference runs
    them: vram_mode.py:24-28, sd_xl_base.yaml:5)."""
    from .sgm_hip.sampling import DiffusionEngine
    from .sgm_hip.unet import UNetModel as SgmUNet
    unet = SgmUNet(**(unet_cfg or SDXL_UNET))
    vae = AutoencoderKL(vae_dd or SDXL_VAE_DD, None, 4)
    if fill:
        synth_fill_(unet, seed, prefix="sgm_unet.")
        synth_fill_(vae, seed, prefix="vae.")
    eng = DiffusionEngine(unet, vae, 0.13025)
    eng.model.to(unet_dtype)
    eng.first_stage_model.to(vae_dtype)
    return eng.to(device).eval()


def build_synthetic_sdxl_refiner(unet_cfg=None, vae_dd=None, device="cuda", unet_dtype=torch.bfloat16, vae_dtype=torch.float32,
                                 seed: int = 1234, fill: bool = True, first_stage=None):
    """The refiner's DiffusionEngine (sd_xl_refiner.yaml: 2.26 B-parameter UNet, the same first stage and denoiser as the base) with
    name-keyed synthetic weights.  `first_stage`: an existing first-stage model to share (the base engine's), instead of a new one."""
    from .sgm_hip.sampling import DiffusionEngine
    from .sgm_hip.unet import UNetModel as SgmUNet
    unet = SgmUNet(**(unet_cfg or SDXL_REFINER_UNET))
    if fill:
        synth_fill_(unet, seed, prefix="sgm_unet.")
    vae = first_stage
    if vae is None:
        vae = AutoencoderKL(vae_dd or SDXL_VAE_DD, None, 4)
        if fill:
            synth_fill_(vae, seed, prefix="vae.")
        vae.to(vae_dtype)
    eng = DiffusionEngine(unet, vae, 0.13025)
    eng.model.to(unet_dtype)
    return eng.to(device).eval()


# svd_xt_1_1.yaml network_config (scripts/sampling/configs): the SVD-XT video UNet
SVD_XT_UNET = dict(adm_in_channels=768, num_classes="sequential", use_checkpoint=True, in_channels=8, out_channels=4, model_channels=320,
                   attention_resolutions=[4, 2, 1], num_res_blocks=2, channel_mult=[1, 2, 4, 4], num_head_channels=64,
                   use_linear_in_transformer=True, transformer_depth=1, context_dim=1024, spatial_transformer_attn_type="softmax-xformers",
                   extra_ff_mix_layer=True, use_spatial_context=True, merge_strategy="learned_with_images", video_kernel_size=[3, 1, 1])


def build_synthetic_svd(unet_cfg=None, device="cuda", unet_dtype=torch.bfloat16, seed: int = 1234, fill: bool = True):
    """The SVD-XT video UNet (cremage_amd.sgm_hip.video.VideoUNet, 1.52 B parameters at the default configuration) with name-keyed
    synthetic weights.  The network alone: its inputs - CLIP image embedding, VAE-encoded conditioning frames, the fps / motion /
    augmentation vector - are the caller's tensors; the latent frames it denoises go to a VideoDecoder (`build_synthetic_svd_vae` /
    `decode_video` below, or the reference's)."""
    from .sgm_hip.video import VideoUNet
    unet = VideoUNet(**(unet_cfg or SVD_XT_UNET))
    if fill:
        synth_fill_(unet, seed, prefix="svd_unet.")
    return unet.to(unet_dtype).to(device).eval()


# svd_xt_1_1.yaml first_stage_config: the SD VAE encoder and the VideoDecoder on the same ddconfig
SVD_VAE_DD = dict(attn_type="vanilla", double_z=True, z_channels=4, resolution=256, in_channels=3, out_ch=3, ch=128, ch_mult=[1, 2, 4, 4],
                  num_res_blocks=2, attn_resolutions=[], dropout=0.0)


def svd_first_stage_config(dd=None, video_kernel_size=(3, 1, 1), **decoder_kw) -> dict:
    """first_stage_config of configs/svd_xt_vae-hip.yaml as a dict (`dd`: another ddconfig, e.g. a narrower one)"""
    dd = dict(dd or SVD_VAE_DD)
    return {"target": "cremage_amd.sgm_hip.video_vae.AutoencodingEngine",
            "params": {"loss_config": {"target": "torch.nn.Identity"},
                       "regularizer_config": {"target": "cremage_amd.sgm_hip.video_vae.DiagonalGaussianRegularizer"},
                       "encoder_config": {"target": "cremage_amd.ldm_hip.vae.Encoder", "params": dd},
                       "decoder_config": {"target": "cremage_amd.sgm_hip.video_vae.VideoDecoder",
                                          "params": dict(dd, video_kernel_size=list(video_kernel_size), **decoder_kw)}}}


def build_synthetic_svd_vae(dd=None, device="cuda", vae_dtype=torch.float32, seed: int = 1234, fill: bool = True, **decoder_kw):
    """The SVD first stage (cremage_amd.sgm_hip.video_vae.AutoencodingEngine: SD VAE encoder + VideoDecoder) with name-keyed synthetic
    weights - the fill re-randomises the zero-initialised second conv of every time_stack and draws `mix_factor` like any parameter, so
    the temporal branch takes part.  fp32 parameters select the fp32-class kernels, as for the image VAE."""
    from .ldm_hip.latent_diffusion import instantiate_from_config
    fs = instantiate_from_config(svd_first_stage_config(dd, **decoder_kw))
    if fill:
        synth_fill_(fs, seed, prefix="svd_vae.")
    return fs.to(vae_dtype).to(device).eval()


@torch.no_grad()
def decode_video(first_stage, z: torch.Tensor, scale_factor: float = 0.18215, decoding_t: Optional[int] = None) -> torch.Tensor:
    """`DiffusionEngine.decode_first_stage` (sgm/models/diffusion.py:118-136) for a VideoDecoder first stage: latent frames [F, 4, h, w]
    -> frames [F, 3, 8 h, 8 w] fp32, `decoding_t` (en_and_decode_n_samples_a_time) frames per decoder call, all of them when None.
    Each chunk is decoded as ONE video of len(chunk) frames: its frame convs zero-pad at the chunk's ends, exactly as the reference's
    do - chunked and unchunked decodes differ there by construction."""
    z = 1.0 / scale_factor * z
    n = z.shape[0] if not decoding_t else int(decoding_t)
    out = []
    for i in range(0, z.shape[0], n):
        chunk = z[i:i + n]
        out.append(first_stage.decode(chunk, timesteps=len(chunk)))
    return torch.cat(out, dim=0)


def build_synthetic_film(cfg=None, device="cuda", seed: int = 1234, fill: bool = True):
    """The FILM interpolator (cremage_amd.film_hip.Interpolator; `cfg`: its constructor arguments, default the film_net configuration) with
    name-keyed synthetic weights.  fp32 parameters: the only class it runs in."""
    from .film_hip import Interpolator
    m = Interpolator(**dict(cfg or {}))
    if fill:
        synth_fill_(m, seed, prefix="film.")
    return m.to(device).eval()


def build_synthetic_unblur(device="cuda", seed: int = 1234, fill: bool = True):
    """Cremage's face unblur / colorize network (cremage_amd.unblur_hip.UnblurCremageModelV6, 620 M parameters) built on the device and
    filled there module by module with name-keyed synthetic weights.  fp32 parameters: the only class it runs in."""
    from .unblur_hip import UnblurCremageModelV6
    with torch.device(device):
        m = UnblurCremageModelV6()
    if fill:
        synth_fill_(m, seed, prefix="unblur.")
    return m.eval()


def _graphed_unblur(model):
    """The model call as a hipGraph replay: one GraphedModule per model object, kept on it and reused across calls (one capture for the
    [1, 3, 256, 256] face; warm-up, the weight stamp and `strict` are GraphedModule's)."""
    g = getattr(model, "_crg_graphed", None)
    if g is None or g.module is not model:
        from .graphs import GraphedModule
        g = GraphedModule(model, const_args=())
        object.__setattr__(model, "_crg_graphed", g)  # a plain attribute: not a submodule, not in the state dict
    return g


@torch.no_grad()
def unblur_faces(model, image, landmarks, *, glue: str = "host", graph: bool = False):
    """The Face Fixer's "Unblur face" / "Colorize face" on an image whose faces were detected elsewhere (face_unblur.py:227-271): per face
    the five landmarks give the similarity transform onto the 256 x 256 template, the aligned face goes through `model` (the unblur or
    the colorize weights) and is warped back and pasted under its eroded mask.  image: uint8 [H, W, 3] (numpy array or tensor); landmarks:
    [faces, 5, 2].  glue "host": numpy on the host (postprocess.unblur_faces), returns a numpy array.  glue "device": the image is uploaded
    once (a tensor on the device is taken as it is and not modified), the warp and the eroded paste run as kernels
    (postprocess.unblur_faces_device: the host arm's bytes, no download and no stream synchronisation per face) and the result is a uint8
    [H, W, 3] tensor on the model's device; a model on the CPU is a CrgError.  graph=True, in either arm: the model call is a hipGraph
    replay (`cremage_amd.graphs.GraphedModule`, kept on the model object) - the same kernels in the same order, the same bits."""
    from . import postprocess as PP
    from ._lib import CrgError
    dev = next(model.parameters()).device
    glue = _glue(glue)
    if dev.type != "cuda" and (glue == "device" or graph):
        raise CrgError(f"unblur_faces: glue='device' and graph=True need the model on a HIP device, it is on {dev}")
    call = _graphed_unblur(model) if graph else model
    if glue == "host":
        img = image.detach().cpu().numpy() if torch.is_tensor(image) else np.asarray(image)
        return PP.unblur_faces(img, landmarks, call, device=dev)
    img = image.detach().to(dev) if torch.is_tensor(image) else torch.from_numpy(np.ascontiguousarray(np.asarray(image))).to(dev)
    with torch.cuda.device(dev):
        return PP.unblur_faces_device(img, landmarks, call)


def colorize_faces(model, image, landmarks, *, glue: str = "host", graph: bool = False):
    """`unblur_faces` with the colorize weights in `model`: the reference runs the same class and the same glue for both buttons
    (face_unblur.py:201-224)."""
    return unblur_faces(model, image, landmarks, glue=glue, graph=graph)


def build_synthetic_hed(device="cuda", seed: int = 1234, fill: bool = True):
    """ControlNet's HED network (cremage_amd.annotator_hip.ControlNetHED_Apache2, 14.7 M parameters) with name-keyed synthetic weights
    (prefix "hed."), its five projections scaled by 1 / 16 so that the edge map is not saturated (tests/_hed_cases.fill_ documents the
    measurement).  fp32 parameters: the only class it runs in."""
    from .annotator_hip import ControlNetHED_Apache2
    m = ControlNetHED_Apache2()
    if fill:
        synth_fill_(m, seed, prefix="hed.")
        with torch.no_grad():
            for k in range(1, 6):
                proj = getattr(m, f"block{k}").projection
                proj.weight.mul_(1.0 / 16.0)
                proj.bias.mul_(1.0 / 16.0)
    return m.to(device).eval()


ANNOTATOR_KINDS = {"hed": "hed", "HED": "hed", "fake_scribble": "fake_scribble", "Fake scribble": "fake_scribble", "scribble": "scribble",
                   "Scribble": "scribble"}  # ours and the menu names of tools/control_net_annotator.py


@torch.no_grad()
def annotate(image, kind: str, *, image_resolution: int = 512, model=None, glue: str = "host"):
    """Cremage's ControlNet Annotator tool for its "HED", "Fake scribble" and "Scribble" entries (annotator_wrapper.py generate_hed :190-201,
    generate_fake_scribble :142-165, generate_scribble :168-187), step by step: the RGB -> BGR flip the wrapper puts in front of every
    detector - HED is an RGB-input model and still gets BGR, as in the reference -, HWC3, resize_image to `image_resolution`, the detector,
    and for the fake scribble the host post-processing (nms, blur, thresholds).  image: a PIL image or uint8 [H, W, C] (numpy array or
    tensor), RGB.  model: the HED network (`build_synthetic_hed` or a loaded ControlNetHED.pth) for "hed" and "fake_scribble".
    Returns "hed": uint8 [H', W']; "fake_scribble", "scribble": uint8 [H', W', 3].  glue "host" (default): only the network runs on the
    device, numpy arrays are returned.  glue "device": the image stays on the GPU from the resized bytes to the edge map (ops.hed_fuse);
    "hed" then returns a uint8 tensor on the device - the same bytes -, the fake scribble's post-processing stays on the host."""
    from . import postprocess as PP
    from ._lib import CrgError
    from .annotator_hip import HEDdetector
    try:
        kind = ANNOTATOR_KINDS[kind]
    except KeyError:
        raise ValueError(f"unknown annotator {kind!r} (one of {sorted(ANNOTATOR_KINDS)})")
    glue = _glue(glue)
    if torch.is_tensor(image):
        img = image.detach().cpu().numpy()
    else:
        img = np.asarray(image)
    if img.dtype != np.uint8 or img.ndim not in (2, 3):
        raise ValueError(f"annotate: a uint8 [H, W, C] image expected, got {img.dtype} {img.shape}")
    if img.ndim == 3:
        img = img[:, :, ::-1]  # RGB to BGR (:30)
    img = PP.resize_for_annotator(PP.hwc3(np.ascontiguousarray(img)), image_resolution)
    if kind == "scribble":
        return PP.scribble_map(img)
    if model is None:
        raise CrgError(f"annotate: {kind!r} needs the HED network (model=)")
    dev = next(model.parameters()).device
    if dev.type != "cuda":
        raise CrgError(f"annotate: the HED network must live on a HIP device, it is on {dev}")
    with torch.cuda.device(dev):
        edge = HEDdetector(model, glue=glue)(np.ascontiguousarray(img))
    if kind == "hed":
        return edge
    if torch.is_tensor(edge):
        edge = edge.cpu().numpy()
    return PP.fake_scribble_from_hed(edge)


def control_hint(map_u8, batch: int, device) -> torch.Tensor:
    """A detected map as the control image txt2img(hint=) takes: fp32 [batch, 3, H, W] in [0, 1] - image_generator.py:832-835 without the
    file round trip (cv2.imread hands back three channels whatever the file holds: HWC3).  map_u8: uint8 [H, W] or [H, W, 3], numpy
    array or tensor."""
    from . import postprocess as PP
    if torch.is_tensor(map_u8):
        m = map_u8.detach()
        if m.dtype != torch.uint8 or m.dim() not in (2, 3):
            raise ValueError(f"control_hint: a uint8 [H, W] or [H, W, 3] map expected, got {m.dtype} {tuple(m.shape)}")
        if m.dim() == 2:
            m = m[:, :, None].expand(-1, -1, 3)
        control = m.to(device).float() / 255.0
    else:
        control = torch.from_numpy(PP.hwc3(np.ascontiguousarray(np.asarray(map_u8))).copy()).float().to(device) / 255.0
    if control.shape[2] != 3:
        raise ValueError(f"control_hint: three channels expected, got {tuple(control.shape)}")
    return control[None].expand(int(batch), -1, -1, -1).permute(0, 3, 1, 2).contiguous()


def film_schedule(inter_frames: int):
    """The order in which the reference fills the `inter_frames` frames between two given ones, as a list of model calls
    (left slot, right slot, target slot, dt).  Slot k of 0 .. inter_frames + 1 sits at time k / (inter_frames + 1) on an fp32 time axis;
    slots 0 and inter_frames + 1 are the given frames.  One call per open slot: among all pairs of (two neighbouring frames that exist
    already, open slot), the pair whose slot lies closest to the midpoint between the two frames wins - the measure is the fp32 value of
    |(t - a) / (b - a) - 1 / 2| for slot time t and frame times a, b, and of equal values the first counts, pairs of frames walked in
    time order and open slots in time order inside each.  The call predicts the slot from those two frames at dt = (t - a) / (b - a),
    fp32.  For three frames: the middle one, then the two quarters, each at dt = 0.5.  Pinned against what the reference's
    `_interpolate_two_frames` really calls (tests/golden/film_schedule.npz)."""
    import bisect
    at = torch.linspace(0, 1, inter_frames + 2).numpy()  # the fp32 time of every slot; np.float32 scalars keep the arithmetic below in fp32
    mid = np.float32(0.5)
    have, missing, calls = [0, inter_frames + 1], list(range(1, inter_frames + 1)), []
    while missing:
        pick = None  # (measure, left, right, slot)
        for left, right in zip(have, have[1:]):
            for slot in missing:
                measure = abs((at[slot] - at[left]) / (at[right] - at[left]) - mid)
                if pick is None or measure < pick[0]:
                    pick = (measure, left, right, slot)
        _, left, right, slot = pick
        calls.append((left, right, slot, float((at[slot] - at[left]) / (at[right] - at[left]))))
        missing.remove(slot)
        bisect.insort(have, slot)
    return calls


def film_pad_region(height: int, width: int, align: int):
    """Zero padding that brings a height x width frame up to multiples of `align`, centred, with the odd pixel (if any) after the frame:
    ((top, bottom, left, right), [y1, x1, y2, x2]) - the second is where the frame lies inside the padded one (the crop that undoes the
    padding).  The geometry of the reference's `pad_batch`; a 30 x 50 frame at 64 gets (17, 17, 7, 7)."""
    def around(size):
        lack = -size % align
        return lack // 2, lack - lack // 2

    (top, bottom), (left, right) = around(height), around(width)
    return (top, bottom, left, right), [top, left, top + height, left + width]


@torch.no_grad()
def interpolate_frames(model, frames: torch.Tensor, inter_frames: int = 3, *, as_uint8: bool = False, signed: bool = False) -> torch.Tensor:
    """The Video Generator's second stage, `inference_multiple_frames(..., interpolation_frames=inter_frames, half=False)` without its
    file and mp4 ends: frames [T, 3, H, W] fp32 in [0, 1], RGB, on the model's device -> the (T - 1) (inter_frames + 1) + 1 frames of the
    slowed-down clip.  Every pair is padded to the model's alignment (`model.align` = 2 ** (pyramid_levels - 1) = the reference's 64)
    with zeros as util.pad_batch does, filled in the order of `film_schedule` with one batch-1 model call per new frame - each
    prediction clamped to [0, 1] before it may serve as a source - and cropped back; the first frame of every pair but the first is dropped.
    `signed`: the frames are decode_video's [-1, 1] output and are mapped by clamp((x + 1) / 2, 0, 1) first (the reference goes through
    8-bit files there; this does not round).  `as_uint8`: (x * 255).byte(), which truncates as the reference does; still RGB, [T', 3, H, W]."""
    if frames.dim() != 4 or frames.shape[1] != 3 or frames.shape[0] < 2:
        raise ValueError(f"interpolate_frames: at least two [3, H, W] frames expected, got {tuple(frames.shape)}")
    if inter_frames < 0:
        raise ValueError(f"interpolate_frames: inter_frames = {inter_frames}")
    frames = frames.float()
    if signed:
        frames = ((frames + 1.0) / 2.0).clamp(0.0, 1.0)
    T, _, H, W = frames.shape
    (top, bottom, left, right), (y1, x1, y2, x2) = film_pad_region(H, W, int(getattr(model, "align", 64)))
    padded = torch.nn.functional.pad(frames, (left, right, top, bottom))
    schedule = film_schedule(inter_frames)
    out = []
    for i in range(1, T):
        slots = {0: padded[i - 1:i], inter_frames + 1: padded[i:i + 1]}
        for lo, hi, tgt, dt in schedule:
            slots[tgt] = model(slots[lo], slots[hi], frames.new_full((1, 1), dt)).clamp(0, 1).float()
        out += [slots[k] for k in range(0 if i == 1 else 1, inter_frames + 2)]
    video = torch.cat(out, dim=0)[:, :, y1:y2, x1:x2]
    return (video * 255).byte() if as_uint8 else video.contiguous()


@torch.no_grad()
def img2vid_latents(engine, c: dict, uc: dict, *, num_frames: int, steps: int = 30, min_scale: float = 1.0, max_scale: float = 2.5,
                    height: int = 576, width: int = 1024, x0: Optional[torch.Tensor] = None, seed: int = 0,
                    sigma_max: float = 700.0) -> torch.Tensor:
    """The Video Generator's sampling call (svd_video_generator.py: EulerEDMSampler on EDMDiscretization, LinearPredictionGuider,
    VScalingWithEDMcNoise) on the HIP VideoUNet `engine` (build_synthetic_svd, or a loaded one): returns the latent frames
    [(b t), 4, height / 8, width / 8] for the reference's VideoDecoder.  c / uc: "crossattn" [(b t), M, 1024], "vector" [(b t), 768],
    "concat" [(b t), 4, h, w]; `x0`: unit-variance start noise (default: torch.randn from `seed`)."""
    from .sgm_hip.video_sampling import sample_video_latents
    frames = c["crossattn"].shape[0]
    if frames % num_frames:
        raise ValueError(f"img2vid_latents: {frames} conditioning rows are no whole number of videos of {num_frames} frames")
    dev = c["crossattn"].device
    if x0 is None:
        g = torch.Generator(device="cpu").manual_seed(seed)
        x0 = torch.randn((frames, 4, height // 8, width // 8), generator=g).to(dev)
    return sample_video_latents(engine, x0.float(), c, uc, num_frames=num_frames, steps=steps, min_scale=min_scale, max_scale=max_scale,
                                sigma_max=sigma_max)


@torch.no_grad()
def txt2img_sdxl(eng, c: dict, uc: dict, *, steps: int = 30, cfg_scale: float = 5.0, height: int = 1024, width: int = 1024,
                 x0: Optional[torch.Tensor] = None, decode: bool = True, sampler: str = "euler_edm", stage2strength: Optional[float] = None,
                 discretization: str = "legacy_ddpm", sampler_options: Optional[dict] = None):
    """run_txt2img -> do_sample (modules/sdxl/sdxl_pipeline/sdxl_image_generator_utils.py:559-772): randn [b,4,H/8,W/8]
    (:695), sampler(denoiser, randn, cond=c, uc=uc) (:707), decode_first_stage in fp32 (:727-734), clamp((x+1)/2, 0, 1).
    c / uc: {"crossattn": [b,77,2048], "vector": [b,2816]}.  `sampler`: a key of sgm_hip.sampling.SGM_SAMPLERS or Cremage's name for
    it ("HeunEDM", ...); `stage2strength`: the refiner strength of a two-stage run, whose base stage stops early
    (Txt2NoisyDiscretizationWrapper); `discretization`: "legacy_ddpm" or "edm"; `sampler_options`: Cremage's sampler preferences
    (sgm_hip.sampling.SAMPLER_OPTION_DEFAULTS)."""
    b = c["crossattn"].shape[0]
    if x0 is None:
        x0 = torch.randn((b, 4, height // 8, width // 8), device=c["crossattn"].device)
    samples = eng.sample(x0, c, uc, steps, cfg_scale, sampler=sampler, stage2strength=stage2strength, discretization=discretization,
                         options=sampler_options)
    if not decode:
        return None, samples
    x = eng.decode_first_stage(samples)
    return ops.affine_cast(x, 0.5, 0.5, torch.float32, 0.0, 1.0), samples


@torch.no_grad()
def img2img_sdxl(eng, init_image: torch.Tensor, c: dict, uc: dict, *, steps: int = 30, strength: float = 0.3, cfg_scale: float = 5.0,
                 enc_noise: Optional[torch.Tensor] = None, fwd_noise: Optional[torch.Tensor] = None, decode: bool = True,
                 sampler: str = "euler_edm", stage2strength: Optional[float] = None, discretization: str = "legacy_ddpm",
                 sampler_options: Optional[dict] = None):
    """run_img2img -> do_img2img (sdxl_image_generator_utils.py:775-1025); with strength 0.3 on a face crop this is the second
    pass of the auto-face-fix (modules/sdxl/face_img2img... -> the same do_img2img).  init_image [b,3,H,W] in [-1,1].
    `sampler` / `stage2strength` / `discretization` / `sampler_options` as in txt2img_sdxl."""
    samples = eng.img2img(init_image, c, uc, steps, strength, cfg_scale, enc_noise=enc_noise, fwd_noise=fwd_noise, sampler=sampler,
                          stage2strength=stage2strength, discretization=discretization, options=sampler_options)
    if not decode:
        return None, samples
    x = eng.decode_first_stage(samples)
    return ops.affine_cast(x, 0.5, 0.5, torch.float32, 0.0, 1.0), samples


@torch.no_grad()
def txt2img_sdxl_hires(eng, c: dict, uc: dict, *, steps: int = 30, cfg_scale: float = 5.0, height: int = 1024, width: int = 1024,
                       factor: float = 2.0, strength: float = 0.3, upscaler: str = "latent", c_hires: Optional[dict] = None,
                       uc_hires: Optional[dict] = None, x0: Optional[torch.Tensor] = None, fwd_noise: Optional[torch.Tensor] = None,
                       enc_noise: Optional[torch.Tensor] = None, sampler: str = "euler_edm", discretization: str = "legacy_ddpm",
                       sampler_options: Optional[dict] = None, decode: bool = True, resample: str = "host"):
    """SDXL hires-fix (sdxl_image_generator.py:166-230): txt2img at (height, width), then an img2img pass at `strength` on the result
    upscaled by `factor` (run_img2img -> do_img2img, sdxl_image_generator_utils.py:986-1017, which adds noise).  `upscaler`:
      "latent"  - bilinear F.interpolate of the base latents, no VAE in between (skip_encode): DiffusionEngine.img2img_latent, on
                  fp32 device latents one launch for the upscale and the noising.
      "lanczos" - decode, postprocess.upscale_uint8 (an APPROXIMATION of the reference's cv2.INTER_LANCZOS4, see there), then
                  DiffusionEngine.img2img (encode with `enc_noise`, noise, sample).
    `c_hires` / `uc_hires`: the conditioning of the second pass.  The reference rebuilds the `vector` conditioning there with the
    upscaled size as original / target size (run_img2img :265-283); the conditioner is PyTorch and outside this package, so the caller
    hands in what it gives.  None reuses c / uc - which DIFFERS from Cremage: the size embedding then still says (height, width).
    The reference runs the second pass one image at a time with a fresh randn each; here the batch runs at once - the same arithmetic
    per image - and `fwd_noise` ([b,4,H*factor/8,W*factor/8]) is the noise of the whole batch.  Both passes use `sampler`,
    `discretization` and `sampler_options` (as in txt2img_sdxl).  `resample`: where the "lanczos" upscaler runs, as in txt2img_hires.
    Returns (images or None, latents, base latents)."""
    from . import postprocess as PP
    upscaler = _upscaler(upscaler)
    resample = _resampler(resample)
    c2, uc2 = (c if c_hires is None else c_hires), (uc if uc_hires is None else uc_hires)
    smp = dict(sampler=sampler, discretization=discretization, options=sampler_options)
    first, base = txt2img_sdxl(eng, c, uc, steps=steps, cfg_scale=cfg_scale, height=height, width=width, x0=x0,
                               decode=upscaler == "lanczos", sampler=sampler, discretization=discretization,
                               sampler_options=sampler_options)
    if upscaler == "latent":
        samples = eng.img2img_latent(base, c2, uc2, steps, strength, cfg_scale, fwd_noise=fwd_noise, factor=factor, **smp)
    else:
        scaled = _lanczos_scaled(PP, first, int(width * factor), int(height * factor), resample, True)
        samples = eng.img2img(scaled, c2, uc2, steps, strength, cfg_scale, enc_noise=enc_noise, fwd_noise=fwd_noise, **smp)
    if not decode:
        return None, samples, base
    x = eng.decode_first_stage(samples)
    return ops.affine_cast(x, 0.5, 0.5, torch.float32, 0.0, 1.0), samples, base


@torch.no_grad()
def refine_sdxl(refiner, z: torch.Tensor, c2: dict, uc2: dict, *, steps: int, strength: float, cfg_scale: float, sampler: str = "dpmpp2m",
                decode: bool = True, discretization: str = "legacy_ddpm", sampler_options: Optional[dict] = None):
    """The refiner stage on base latents z [b,4,H/8,W/8] (apply_refiner, sdxl_image_generator.py:307-347): Img2Img-pruned schedule
    of `steps` at `strength`, no added noise, then decode and clamp((x+1)/2, 0, 1).  c2 / uc2: the refiner conditioner's output,
    {"crossattn": [b,77,1280], "vector": [b,2560]}.  `sampler` / `discretization` / `sampler_options` as in txt2img_sdxl.  Returns
    (images or None, latents)."""
    samples = refiner.refine(z, c2, uc2, steps, strength, cfg_scale, sampler=sampler, discretization=discretization,
                             options=sampler_options)
    if not decode:
        return None, samples
    x = refiner.decode_first_stage(samples)
    return ops.affine_cast(x, 0.5, 0.5, torch.float32, 0.0, 1.0), samples


@torch.no_grad()
def txt2img_sdxl_refined(base, refiner, c: dict, uc: dict, c2: dict, uc2: dict, *, steps: int = 30, refiner_strength: float = 0.15,
                         cfg_scale: float = 5.0, sampler: str = "dpmpp2m", height: int = 1024, width: int = 1024,
                         x0: Optional[torch.Tensor] = None, decode: bool = True, discretization: str = "legacy_ddpm",
                         sampler_options: Optional[dict] = None):
    """SDXL txt2img with the refiner stage (sdxl_use_refiner, sdxl_image_generator.py:420-424, :555-635): the base samples with the
    schedule's last sigmas dropped (Txt2Noisy, stage2strength = refiner_strength) and is not decoded; the refiner continues from its
    latents (refine_sdxl) and its first stage decodes.  refiner_strength == 0 turns the refiner off, as the reference does: the
    result is txt2img_sdxl's.  Both stages use `sampler`, `discretization` and `sampler_options` (as in txt2img_sdxl).  Returns
    (images or None, base latents, final latents)."""
    smp = dict(sampler=sampler, discretization=discretization, sampler_options=sampler_options)
    if refiner_strength == 0:
        images, samples = txt2img_sdxl(base, c, uc, steps=steps, cfg_scale=cfg_scale, height=height, width=width, x0=x0, decode=decode,
                                       **smp)
        return images, samples, samples
    _, z = txt2img_sdxl(base, c, uc, steps=steps, cfg_scale=cfg_scale, height=height, width=width, x0=x0, decode=False,
                        stage2strength=refiner_strength, **smp)
    images, samples = refine_sdxl(refiner, z, c2, uc2, steps=steps, strength=refiner_strength, cfg_scale=cfg_scale, decode=decode, **smp)
    return images, z, samples


@torch.no_grad()
def txt2img_sdxl_facefix(eng, c: dict, uc: dict, boxes, *, steps: int = 30, cfg_scale: float = 5.0, height: int = 1024, width: int = 1024,
                         fix_size: Optional[int] = None, strength: float = 0.3, x0: Optional[torch.Tensor] = None,
                         enc_noise: Optional[torch.Tensor] = None, fwd_noise: Optional[torch.Tensor] = None, paste: bool = True,
                         sampler: str = "euler_edm", discretization: str = "legacy_ddpm", sampler_options: Optional[dict] = None,
                         paste_mode: str = "paste"):
    """BASELINE config 5: SDXL txt2img, then the auto-face-fix second pass on one region per image - the UNet RE-ENTRY on a crop.

    Reference flow (modules/sdxl/sdxl_pipeline/sdxl_image_generator_utils.py:559-772 txt2img, then per detected face
    modules/face_detection/face_img2img.py:57-235 -> do_img2img :906-1025): crop the face box, bring the crop to the generation
    size, img2img it with strength 0.3 (encode -> noise to sigma_0 of the pruned schedule -> Euler-EDM over the last
    int(0.3 * steps) sigmas -> decode), bring it back to the box size and paste it over the first-pass image.
    In scope here is the numeric path (both UNet passes, VAE encode / decode); the glue around it is deliberately plain PyTorch:
    `boxes` = one (top, left, size) per image instead of the face detector (out of scope), the two resizes are
    F.interpolate(bilinear, antialias off) instead of cv2 Lanczos (not built), the paste is a hard-edged copy.
    Both passes use `sampler`, `discretization` and `sampler_options` (as in txt2img_sdxl).  `paste_mode` "poisson": the paste is
    postprocess's gradient-domain one on the device (ops.poisson_clone on the images quantised to uint8 as unit_tensor_to_pil does, so
    the whole result is then a multiple of 1/255), the stated approximation of the reference's cv.seamlessClone; the default stays the copy.
    Returns (final images [b,3,H,W] in [0,1], first-pass images, second-pass crops at `fix_size`)."""
    import torch.nn.functional as F
    from . import postprocess as PP
    paste_mode = _paste_mode(PP, paste_mode)
    if paste_mode == "seamless":
        raise NotImplementedError("cv.seamlessClone (Poisson blending) needs OpenCV, which this build cannot import or pin against")
    smp = dict(sampler=sampler, discretization=discretization, sampler_options=sampler_options)
    first, _ = txt2img_sdxl(eng, c, uc, steps=steps, cfg_scale=cfg_scale, height=height, width=width, x0=x0, **smp)
    fix = fix_size or height
    crops = torch.stack([F.interpolate(first[i:i + 1, :, t:t + sz, l:l + sz], size=(fix, fix), mode="bilinear", align_corners=False)[0]
                         for i, (t, l, sz) in enumerate(boxes)])
    fixed, _ = img2img_sdxl(eng, crops * 2.0 - 1.0, c, uc, steps=steps, strength=strength, cfg_scale=cfg_scale, enc_noise=enc_noise,
                            fwd_noise=fwd_noise, **smp)
    out = first.clone()
    if paste and paste_mode == "poisson":
        quantise = lambda v: (255.0 * v.float().clamp(0, 1)).to(torch.uint8)
        u8 = quantise(first)
        for i, (t, l, sz) in enumerate(boxes):
            face = quantise(F.interpolate(fixed[i:i + 1], size=(sz, sz), mode="bilinear", align_corners=False))
            ops.poisson_clone(u8[i:i + 1], face, (l, t), PP.POISSON_MARGIN)
        out = PP.u8_to_unit_device(u8).to(first.dtype)
    elif paste:
        for i, (t, l, sz) in enumerate(boxes):
            out[i, :, t:t + sz, l:l + sz] = F.interpolate(fixed[i:i + 1], size=(sz, sz), mode="bilinear", align_corners=False)[0]
    return out, first, fixed


@torch.no_grad()
def face_fix_sdxl(eng, images: torch.Tensor, faces, c: dict, uc: dict, *, steps: int = 30, strength: float = 0.3, cfg_scale: float = 5.0,
                  target_edge_len: int = 1024, enc_noise: Optional[torch.Tensor] = None, fwd_noise: Optional[torch.Tensor] = None,
                  sampler: str = "euler_edm", discretization: str = "legacy_ddpm", sampler_options: Optional[dict] = None,
                  resample: str = "host", paste_mode: str = "paste"):
    """The auto-face-fix second pass with the REFERENCE's host-side glue (cremage_amd.postprocess: buffer / clamp / aspect-preserving
    Lanczos resize / white padding / un-pad / resize back / paste, face_detector_engine.py:152-288) around the UNet re-entry
    (`img2img_sdxl`, strength 0.3).  images [b,3,H,W] in [0,1]; faces[i] = list of (x, y, w, h) boxes of image i (the detector is out
    of scope).  Differences from the reference that remain: plain paste instead of cv.seamlessClone (no OpenCV here; `paste_mode`
    "poisson" is its stated approximation, postprocess.poisson_clone_host - on the device ops.poisson_clone, bytes within 1), and one
    conditioning row per image instead of a gender-prefixed prompt.  `sampler` / `discretization` / `sampler_options` as in
    txt2img_sdxl.  `resample` ("host", the default, or "device"): "device" keeps the image on the GPU (postprocess.face_fix_device: two
    launches of ops.resample_u8 per face instead of two transfers, two synchronisations and the PIL calls) and returns the same
    tensor to the bit.  Returns [b,3,H,W] in [0,1] on the images' device."""
    from . import postprocess as PP
    resample, paste_mode = _resampler(resample), _paste_mode(PP, paste_mode)
    out = []
    for i in range(images.shape[0]):
        ci = {k: v[i:i + 1] for k, v in c.items()}
        uci = {k: v[i:i + 1] for k, v in uc.items()}

        def i2i(x):
            y, _ = img2img_sdxl(eng, x.to(images.device), ci, uci, steps=steps, strength=strength, cfg_scale=cfg_scale,
                                enc_noise=enc_noise[i:i + 1] if enc_noise is not None else None,
                                fwd_noise=fwd_noise[i:i + 1] if fwd_noise is not None else None, sampler=sampler,
                                discretization=discretization, sampler_options=sampler_options)
            return y
        out.append(_face_fix_one(PP, images[i], faces[i], i2i, target_edge_len, resample, paste_mode))
    return torch.stack(out).to(images.device)


def _paste_mode(PP, name: str) -> str:
    if name != "seamless" and name not in PP.PASTE_MODES:  # "seamless" raises NotImplementedError where the paste happens
        raise ValueError(f"unknown paste mode {name!r} (one of {list(PP.PASTE_MODES)})")
    return name


def _face_fix_one(PP, image: torch.Tensor, faces, i2i: Callable, target_edge_len: int, resample: str, paste_mode: str = "paste") -> torch.Tensor:
    """One image through postprocess.face_fix (PIL, host) or face_fix_device -> [3,H,W] fp32, ((u / 255 * 2 - 1) + 1) * 0.5 either way."""
    if resample == "device":
        u8 = PP.face_fix_device(image, faces, i2i, target_edge_len, paste_mode)
        return (PP.u8_to_unit_device(u8[None], (2.0, -1.0))[0] + 1.0) * 0.5
    pil = PP.face_fix(PP.unit_tensor_to_pil(image), faces, i2i, target_edge_len, paste_mode)
    return (PP.pil_to_unit_tensor(pil)[0] + 1.0) * 0.5


@torch.no_grad()
def face_fix_sd15(ldm: LatentDiffusion, images: torch.Tensor, faces, c: torch.Tensor, uc: Optional[torch.Tensor], *, steps: int = 20,
                  strength: float = 0.3, cfg_scale: float = 7.5, target_edge_len: int = 512, enc_noise: Optional[torch.Tensor] = None,
                  fwd_noise: Optional[torch.Tensor] = None, resample: str = "host", paste_mode: str = "paste"):
    """The SD1.5 auto-face-fix second pass (face_detector_engine.py `face_fix_generator_model_type` SD 1.5: the same crop / pad / paste
    glue as face_fix_sdxl around `img2img`, whose sampler the reference forces to DDIM).  images [b,3,H,W] in [0,1]; faces[i] = list of
    (x, y, w, h) boxes of image i; c / uc: [b, 77*n, 768], one conditioning row per image; enc_noise [b,4,edge/8,edge/8] / fwd_noise: row i
    is the noise of every face of image i.  `resample` and `paste_mode` as in face_fix_sdxl.  Returns [b,3,H,W] in [0,1] on the images' device."""
    from . import postprocess as PP
    resample, paste_mode = _resampler(resample), _paste_mode(PP, paste_mode)
    out = []
    for i in range(images.shape[0]):
        def i2i(x, i=i):
            y, _ = img2img(ldm, x.to(images.device), c[i:i + 1], uc[i:i + 1] if uc is not None else None, steps=steps, strength=strength,
                           cfg_scale=cfg_scale, enc_noise=enc_noise[i:i + 1] if enc_noise is not None else None,
                           fwd_noise=fwd_noise[i:i + 1] if fwd_noise is not None else None)
            return y
        out.append(_face_fix_one(PP, images[i], faces[i], i2i, target_edge_len, resample, paste_mode))
    return torch.stack(out).to(images.device)


# ---------------------------------------------------------------------------------------------- spot inpainting (tools/spot_inpainter.py)
GLUES = ("host", "device")  # where the pixel steps around the inpainting UNet run: PIL / numpy on the host, or the HIP twins


def _glue(name: str) -> str:
    if name not in GLUES:
        raise ValueError(f"unknown glue {name!r} (one of {list(GLUES)})")
    return name


def _u8_hwc_device(image, device, channels: bool) -> torch.Tensor:
    """PIL image or uint8 tensor -> device uint8 [H, W, 3] (channels) or [H, W] (grey, PIL's "L")"""
    if not torch.is_tensor(image):
        image = torch.from_numpy(np.array(image.convert("RGB" if channels else "L")))
    if image.dtype != torch.uint8 or image.dim() != (3 if channels else 2):
        raise ValueError(f"uint8 {'[H, W, C]' if channels else '[H, W]'} tensor expected, got {image.dtype} {tuple(image.shape)}")
    return image.to(device)


@torch.no_grad()
def inpaint_image(ldm: LatentDiffusion, image, mask, c: torch.Tensor, uc: Optional[torch.Tensor], *, width: int, height: int, steps: int = 50,
                  cfg_scale: float = 7.5, eta: float = 1.0, seed: Optional[int] = None, glue: str = "host",
                  noise_sampler: Optional[Callable] = None, enc_noise: Optional[torch.Tensor] = None):
    """One image through the reference's inpainting generate call (inpaint.py:110-147 and :357-399 around `inpaint`): the image and
    the mask (white = repaint) are resized and white-padded to (width, height) rounded up to multiples of 64 when their size differs
    from it (postprocess.resize_with_padding - the padding of the mask is white too), make_batch_sd, the 9-channel UNet under DDIM,
    the blurred-mask composite over the padded original and the crop to the padding's inner box.  c / uc: one conditioning row.
    glue "host" (the default): PIL images in, PIL RGB image out, the pixel steps in PIL / numpy.  glue "device": the image (PIL, or
    uint8 [H, W, 3 or 4] tensor) and the mask (PIL, read as "L", or uint8 [H, W]) go to the device once and stay there - two launches
    of ops.resample_u8 for the padding, ops.blur_blend_u8 for the composite - and the result is a device uint8 [h, w, 3] tensor with
    the host arm's bytes.  The device arm reads channels 0-2 of the image and a GREY mask: PIL premultiplies a non-opaque alpha
    before it resizes, which is not restated."""
    from . import postprocess as PP
    glue = _glue(glue)
    dev = ldm.device
    pw, ph = PP.bbox_for_multiple_of_64(width, height)
    kw = dict(steps=steps, cfg_scale=cfg_scale, eta=eta, seed=seed, noise_sampler=noise_sampler, enc_noise=enc_noise)
    if glue == "host":
        bbox = None
        if image.size != (pw, ph):
            image, bbox = PP.resize_with_padding(image, pw, ph)
        if mask.size != (pw, ph):
            mask, _ = PP.resize_with_padding(mask, pw, ph)
        img, m, _ = PP.inpaint_batch(image, mask)
        out, _ = inpaint(ldm, img.to(dev), m.to(dev), c, uc, **kw)
        return PP.composite_inpaint(image, PP.unit_tensor_to_pil(out[0]), mask, bbox)
    orig = _u8_hwc_device(image, dev, True)[..., :3]
    grey = _u8_hwc_device(mask, dev, False)
    bbox = None
    if (orig.shape[1], orig.shape[0]) != (pw, ph):
        nw, nh, px, py = PP.resize_with_padding_plan(orig.shape[1], orig.shape[0], pw, ph)
        padded = torch.empty((ph, pw, 3), dtype=torch.uint8, device=dev)
        ops.resample_u8(orig.permute(2, 0, 1)[None], (nh, nw), out=padded.permute(2, 0, 1)[None], out_offset=(px, py), fill=255.0)
        orig, bbox = padded, (px, py, px + nw, py + nh)
    if (grey.shape[1], grey.shape[0]) != (pw, ph):
        nw, nh, px, py = PP.resize_with_padding_plan(grey.shape[1], grey.shape[0], pw, ph)
        padded = torch.empty((ph, pw), dtype=torch.uint8, device=dev)
        ops.resample_u8(grey[None, None], (nh, nw), out=padded[None, None], out_offset=(px, py), fill=255.0)
        grey = padded
    img = PP.u8_to_unit_device(orig.permute(2, 0, 1)[None], (2.0, -1.0))  # v / 127.5 - 1 to the bit: 2 (v / 255) is exact
    m = (grey >= 128).to(torch.float32)[None, None]                        # float32(v) / 255 >= 0.5
    out, _ = inpaint(ldm, img, m, c, uc, **kw)
    inpainted = (255.0 * out[0].clamp(0, 1)).to(torch.uint8).permute(1, 2, 0).contiguous()
    return PP.composite_inpaint_device(orig, inpainted, grey, bbox)


@torch.no_grad()
def spot_fix_sd15(ldm: LatentDiffusion, image: torch.Tensor, mask, c: torch.Tensor, uc: Optional[torch.Tensor], *, steps: int = 20,
                  strength: float = 0.5, cfg_scale: float = 7.5, resample: str = "host", boxes=None, target_edge_len: int = 512,
                  enc_noise: Optional[torch.Tensor] = None, fwd_noise: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Spot inpainting with a regular SD1.5 model (spot_inpainter.py "Apply inpainting" without the inpainting checkbox): every
    connected region of the mask gets one `img2img` pass (DDIM, strength 0.5 - the tool's default -, batch 1) through the face-fix
    geometry, and the whole image is blended through the blurred mask after each (postprocess.spot_fix).  image: [3, H, W] in [0, 1]
    on the model's device; mask: HOST uint8 [H, W] (array or tensor; > 127 = repaint); c / uc: [1, 77*n, 768]; `boxes`: (x, y, w, h)
    boxes to use instead of postprocess.mask_boxes(mask) - their order and connectivity are assumptions about cv2 stated there.
    `resample` ("host", the default, or "device"): "device" keeps the image on the GPU between the boxes
    (postprocess.spot_fix_device) and returns the same tensor to the bit.  Returns [3, H, W] in [0, 1] on the image's device."""
    from . import postprocess as PP
    resample = _resampler(resample)
    mask = np.asarray(mask.cpu() if torch.is_tensor(mask) else mask)

    def i2i(x):
        y, _ = img2img(ldm, x.to(image.device), c, uc, steps=steps, strength=strength, cfg_scale=cfg_scale, enc_noise=enc_noise, fwd_noise=fwd_noise)
        return y
    if resample == "device":
        u8 = PP.spot_fix_device(image, mask, i2i, boxes, target_edge_len)
        return (PP.u8_to_unit_device(u8[None], (2.0, -1.0))[0] + 1.0) * 0.5
    pil = PP.spot_fix(PP.unit_tensor_to_pil(image), mask, i2i, boxes, target_edge_len)
    return ((PP.pil_to_unit_tensor(pil)[0] + 1.0) * 0.5).to(image.device)


@torch.no_grad()
def spot_inpaint_sd15(inpaint_ldm: LatentDiffusion, image: torch.Tensor, mask, c: torch.Tensor, uc: Optional[torch.Tensor], *,
                      max_edge_len: int = 768, steps: int = 50, cfg_scale: float = 7.5, eta: float = 1.0, seed: Optional[int] = None,
                      glue: str = "host", noise_sampler: Optional[Callable] = None, enc_noise: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Spot inpainting with the SD1.5 inpainting model (the tool's inpainting checkbox): the window of at most max_edge_len squared
    around every mask region (postprocess.mask_single_box / spot_window) goes through `inpaint_image` at width = height =
    max_edge_len and the patch is pasted at the window's origin (postprocess.spot_inpaint, whose oversize-patch quirk is kept).
    image: [3, H, W] in [0, 1] on the model's device; mask: HOST uint8 [H, W].  `glue` "device" keeps every pixel step on the GPU
    (postprocess.spot_inpaint_device, inpaint_image's device arm) and returns the same tensor to the bit.  Returns [3, H, W] in [0, 1]."""
    from . import postprocess as PP
    glue = _glue(glue)
    mask = np.asarray(mask.cpu() if torch.is_tensor(mask) else mask)

    def fn(crop, mask_crop, edge_len):
        return inpaint_image(inpaint_ldm, crop, mask_crop, c, uc, width=edge_len, height=edge_len, steps=steps, cfg_scale=cfg_scale, eta=eta,
                             seed=seed, glue=glue, noise_sampler=noise_sampler, enc_noise=enc_noise)
    if glue == "device":
        u8 = (255.0 * image.detach().float().clamp(0, 1)).to(torch.uint8).permute(1, 2, 0).contiguous()
        u8 = PP.spot_inpaint_device(u8, mask, fn, max_edge_len)
        return (PP.u8_to_unit_device(u8.permute(2, 0, 1)[None], (2.0, -1.0))[0] + 1.0) * 0.5
    pil = PP.spot_inpaint(PP.unit_tensor_to_pil(image), mask, fn, max_edge_len)
    return ((PP.pil_to_unit_tensor(pil)[0] + 1.0) * 0.5).to(image.device)
