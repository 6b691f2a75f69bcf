"""ORACLE tooling for the hires-fix and ControlNet img2img routes - writes tests/golden/{traj_cn_ddim_img2img, traj_cn_hires_latent,
traj_sdxl_hires_latent}.npz from the reference's own classes (cldm.cldm.ControlLDM, cldm.ddim_hacked.DDIMSampler, Cremage's
Dpmpp2mSampler, the sgm EulerEDMSampler with Img2ImgDiscretizationWrapper), fp32 on the CPU, on the name-keyed synthetic weights and
`synth_input` tensors of oracle/gen_golden.py, whose import stubs and helpers it reuses (that module is imported, not changed).
modules/sd/image_generator.py itself cannot be imported (cv2), so the sampler classes are called directly, composed in the order of
its lines: img2img_sampling :168-190 for ControlNet img2img, :878-932 for the ControlNet latent hires-fix,
sdxl_image_generator.py:166-230 -> do_img2img (sdxl_image_generator_utils.py:986-1017) for SDXL.  All noise and both hint sizes are
explicit arrays in the fixtures; the text conditionings are `synth_input` tensors the tests rebuild from their names.  Only the
.npz files are committed; a rerun reproduces the arrays exactly.

One deviation, forced: the reference's LDMWrapperForKDiffusion wraps whatever conditioning it doubled as {"c_crossattn": [c_in]}
(ldm_wrapper_for_k_diffusion.py:92), so a DICT conditioning reaches ControlLDM.apply_model nested inside a list and torch.cat raises
a TypeError there: the reference cannot run a k-diffusion sampler with a ControlNet as written.  `DictCondWrapper` below hands the
doubled dict on as it is - the same doubling (:67-84), the same guidance (:98) - which is what ddim_hacked does with the two dicts.

    python tools/gen_golden_hires_routes.py [--only NAME ...]
"""
import argparse
import contextlib
import os
import sys
import types

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from oracle import gen_golden as G  # noqa: E402  (installs the import stubs and puts the reference on sys.path)
from oracle.gen_golden import R_ks, R_ksamp, SEED, fp32_forward, save, synth_input  # noqa: E402

from cremage_amd.synth import synth_fill_  # noqa: E402
from ldm.models.diffusion.ldm_wrapper_for_k_diffusion import LDMWrapperForKDiffusion  # noqa: E402
from ldm.modules.distributions.distributions import DiagonalGaussianDistribution  # noqa: E402

CN = dict(B=2, L=8, S=6, cfg=7.5, strength=0.5)


def _quiet():
    R_ks.trange = R_ksamp.trange = lambda *a, **k: range(*a)  # silence tqdm


def _tiny_control_ldm():
    """The reference's ControlLDM on the tiny UNet / VAE of traj_euler: ControlledUnetModel + ControlNet + AutoencoderKL, weights
    under the prefixes pipeline.build_synthetic_control_ldm uses."""
    from cldm.cldm import ControlLDM
    ccfg = {k: v for k, v in G.TINY_UNET.items() if k != "out_channels"}
    ldm = ControlLDM(control_stage_config={"target": "cldm.cldm.ControlNet", "params": dict(hint_channels=3, **ccfg)},
                     control_key="hint", only_mid_control=False,
                     first_stage_config={"target": "ldm.models.autoencoder.AutoencoderKL",
                                         "params": dict(ddconfig=G.TINY_DD, lossconfig={"target": "torch.nn.Identity"}, embed_dim=4)},
                     cond_stage_config={"target": "torch.nn.Identity"},
                     unet_config={"target": "cldm.cldm.ControlledUnetModel", "params": G.TINY_UNET},
                     linear_start=0.00085, linear_end=0.012, timesteps=1000, conditioning_key="crossattn", scale_factor=0.18215,
                     use_ema=False, cond_stage_trainable=False, first_stage_key="jpg", cond_stage_key="txt", image_size=16, channels=4)
    synth_fill_(ldm.model.diffusion_model, SEED, prefix="unet.")
    synth_fill_(ldm.control_model, SEED, prefix="cn.")
    synth_fill_(ldm.first_stage_model, SEED, prefix="vae.")
    return ldm.eval()


@contextlib.contextmanager
def _no_half():
    """cldm.py:54-55, :67-68, :322-323 cast to fp16 whenever a tensor is not on a 'cuda' device: neutralised, the run stays fp32."""
    orig = torch.Tensor.half
    torch.Tensor.half = lambda self, *a, **k: self
    try:
        with fp32_forward(), contextlib.redirect_stdout(open(os.devnull, "w")):
            yield
    finally:
        torch.Tensor.half = orig


def _hint(name, B, edge):
    return synth_input(name, (B, 3, edge, edge), SEED, 0.5).clamp(-1, 1) * 0.5 + 0.5


def _dicts(c, uc, hint):
    return {"c_concat": [hint], "c_crossattn": [c]}, {"c_concat": [hint], "c_crossattn": [uc]}  # image_generator.py:839-846


def g_traj_cn_ddim_img2img():
    """ControlNet img2img (image_generator.py:721-727, :850-875 -> img2img_sampling :168-190): first-stage encoding with explicit
    posterior noise, DDIMControlNetSampler.stochastic_encode and decode with the two dict conditionings."""
    from cldm import ddim_hacked as R_hacked
    R_hacked.tqdm = lambda it, **k: it
    ldm = _tiny_control_ldm()
    B, L, S, cfg = CN["B"], CN["L"], CN["S"], CN["cfg"]
    t_enc = int(CN["strength"] * S)
    c, uc = synth_input("cni2i.c", (B, 77, 96), SEED), synth_input("cni2i.uc", (B, 77, 96), SEED)
    hint = _hint("cni2i.hint", B, 8 * L)
    img_in = synth_input("cni2i.img", (B, 3, 2 * L, 2 * L), SEED, 0.5).clamp(-1, 1)  # TINY_DD has one down level
    enc_noise, fwd_noise = synth_input("cni2i.encnoise", (B, 4, L, L), SEED), synth_input("cni2i.fwdnoise", (B, 4, L, L), SEED)
    dd = R_hacked.DDIMSampler(ldm)
    dd.register_buffer = lambda name, attr: setattr(dd, name, attr)
    cond, ucond = _dicts(c, uc, hint)
    torch.manual_seed(0)
    with _no_half():
        dd.make_schedule(ddim_num_steps=S, ddim_eta=0.0, verbose=False)
        post = DiagonalGaussianDistribution(ldm.first_stage_model.quant_conv(ldm.first_stage_model.encoder(img_in)))
        init_latent = 0.18215 * (post.mean + post.std * enc_noise)  # ddpm.py:575-582
        z_enc = dd.stochastic_encode(init_latent, torch.tensor([t_enc] * B), noise=fwd_noise)
        x = dd.decode(z_enc, cond, t_enc, unconditional_guidance_scale=cfg, unconditional_conditioning=ucond)
        img = ldm.decode_first_stage(x)
    save("traj_cn_ddim_img2img", dict(CN, t_enc=t_enc, seed=SEED, unet=G.TINY_UNET, dd=G.TINY_DD),
         hint=hint, img_in=img_in, enc_noise=enc_noise, fwd_noise=fwd_noise, init_latent=init_latent, z_enc=z_enc, x=x,
         img=img)


class DictCondWrapper(LDMWrapperForKDiffusion):
    """LDMWrapperForKDiffusion for dict conditioning (see the module docstring): the doubled dict goes to the CompVis wrapper as `cond`."""

    def apply_model(self, x, t, **kwargs):
        c, uc, scale = self.c, self.unconditional_conditioning, self.unconditional_guidance_scale
        c_in = {k: [torch.cat([uc[k][i], c[k][i]]) for i in range(len(c[k]))] for k in c}
        e_t_uncond, e_t = self.compviz_model(torch.cat([x] * 2), torch.cat([t] * 2), cond=c_in).chunk(2)
        return e_t_uncond + scale * (e_t - e_t_uncond)


def _prep(s, cond, ucond, cfg, **kw):
    """_sample_common_prep, with the sampler's CFG wrapper replaced by DictCondWrapper."""
    s._sample_common_prep(conditioning=cond, unconditional_guidance_scale=cfg, unconditional_conditioning=ucond, **kw)
    s.ldm_wrapper_model = DictCondWrapper(s.compviz_wrapper_model, cond, ucond, cfg)


def g_traj_cn_hires_latent():
    """ControlNet hires-fix with the latent upscaler (image_generator.py:878-932) and DPM++ 2M: txt2img with the hint, F.interpolate of
    the latents, k-diffusion stochastic_encode, then `denoising_steps` with the hires hint.  Both hints are independent arrays."""
    from tools.gen_golden_sd15_samplers import _cremage_sampler
    _quiet()
    ldm = _tiny_control_ldm()
    B, L, S, cfg, factor = CN["B"], CN["L"], CN["S"], CN["cfg"], 2
    t_enc = int(CN["strength"] * S)
    c, uc = synth_input("cnhires.c", (B, 77, 96), SEED), synth_input("cnhires.uc", (B, 77, 96), SEED)
    x0 = synth_input("cnhires.x0", (B, 4, L, L), SEED)
    hint, hint_hires = _hint("cnhires.hint", B, 8 * L), _hint("cnhires.hint_hires", B, 8 * L * factor)
    fwd_noise = synth_input("cnhires.fwdnoise", (B, 4, factor * L, factor * L), SEED)
    s = _cremage_sampler(ldm, "dpmpp_2m")
    assert s.sqrt_alphas_cumprod.dtype == torch.float32
    with _no_half():
        _prep(s, *_dicts(c, uc, hint), cfg, S=S, batch_size=B, shape=[4, L, L], x0=x0)
        base, _ = s.do_sample()
        up = torch.nn.functional.interpolate(base, scale_factor=factor, mode="bilinear", align_corners=False)
        z_enc = s.stochastic_encode(up, torch.tensor([t_enc] * B), sampling_steps=S, noise=fwd_noise)
        _prep(s, *_dicts(c, uc, hint_hires), cfg, S=S, batch_size=B, shape=[4, factor * L, factor * L], x0=z_enc, denoising_steps=t_enc)
        x, _ = s.do_sample()
        img = ldm.decode_first_stage(x)
    save("traj_cn_hires_latent", dict(CN, factor=factor, t_enc=t_enc, sampler="DPM++ 2M", seed=SEED, unet=G.TINY_UNET, dd=G.TINY_DD),
         x0=x0, hint=hint, hint_hires=hint_hires, fwd_noise=fwd_noise, base=base, up=up, z_enc=z_enc, sigmas=s.sigmas, x=x,
         img=img)


XL = dict(B=2, L=8, S=8, cfg=5.0, factor=1.5, strength=0.5, scale_factor=0.13025)


def g_traj_sdxl_hires_latent():
    """SDXL hires-fix with the latent upscaler (sdxl_image_generator.py:166-230): do_sample with EulerEDMSampler, F.interpolate of
    the latents by 1.5 (8x8 -> 12x12), then do_img2img with skip_encode and add_noise on the Img2Img-pruned schedule
    (sdxl_image_generator_utils.py:986-1017), with the second pass' own `vector` conditioning (run_img2img :265-283)."""
    SU, DN, DZ, GD, SM, WR = G._import_sgm()
    SM.denoising_status_queue = types.SimpleNamespace(put=lambda *a, **k: None)
    from scripts.demo.discretization import Img2ImgDiscretizationWrapper
    unet = SU.UNetModel(**G.TINY_SGM_UNET)
    synth_fill_(unet, SEED, prefix="sgm_unet.")
    model = WR.OpenAIWrapper(unet)
    legacy = {"target": "sgm.modules.diffusionmodules.discretizer.LegacyDDPMDiscretization"}
    den = DN.DiscreteDenoiser(scaling_config={"target": "sgm.modules.diffusionmodules.denoiser_scaling.EpsScaling"}, num_idx=1000,
                              discretization_config=legacy)
    B, L, S, factor = XL["B"], XL["L"], XL["S"], XL["factor"]
    L2 = int(L * factor)

    def sampler():
        return SM.EulerEDMSampler(discretization_config=legacy, num_steps=S, device="cpu",
                                  guider_config={"target": "sgm.modules.diffusionmodules.guiders.VanillaCFG", "params": {"scale": XL["cfg"]}})
    vec = lambda name: synth_input(name, (B, 96), SEED)  # noqa: E731
    ctx_c, ctx_uc = synth_input("xlhires.c", (B, 77, 128), SEED), synth_input("xlhires.uc", (B, 77, 128), SEED)
    c, uc = {"crossattn": ctx_c, "vector": vec("xlhires.cv")}, {"crossattn": ctx_uc, "vector": vec("xlhires.ucv")}
    c2, uc2 = {"crossattn": ctx_c, "vector": vec("xlhires.cv2")}, {"crossattn": ctx_uc, "vector": vec("xlhires.ucv2")}
    x0 = synth_input("xlhires.x0", (B, 4, L, L), SEED)
    fwd_noise = synth_input("xlhires.fwdnoise", (B, 4, L2, L2), SEED)
    denoiser = lambda inp, sigma, cc: den(model, inp, sigma, cc)  # noqa: E731
    ae = G._make_ae(G.TINY_DD)
    with fp32_forward(), contextlib.redirect_stdout(open(os.devnull, "w")):
        base = sampler()(denoiser, x0.clone(), cond=c, uc=uc)
        up = torch.nn.functional.interpolate(base, scale_factor=factor, mode="bilinear", align_corners=False)
        smp = sampler()
        smp.discretization = Img2ImgDiscretizationWrapper(smp.discretization, strength=XL["strength"])
        sigmas = smp.discretization(smp.num_steps)
        noised_z = (up + fwd_noise * sigmas[0]) / torch.sqrt(1.0 + sigmas[0] ** 2.0)
        x = smp(denoiser, noised_z.clone(), cond=c2, uc=uc2)
        img = ae.decode(x / XL["scale_factor"])
    assert tuple(up.shape[-2:]) == (L2, L2)
    save("traj_sdxl_hires_latent", dict(XL, seed=SEED, unet=G.TINY_SGM_UNET, dd=G.TINY_DD),
         cv=c["vector"], ucv=uc["vector"], cv2=c2["vector"], ucv2=uc2["vector"], x0=x0, fwd_noise=fwd_noise,
         base=base, up=up, sigmas=sigmas, noised_z=noised_z, x=x, img=img)


CASES = {"traj_cn_ddim_img2img": g_traj_cn_ddim_img2img, "traj_cn_hires_latent": g_traj_cn_hires_latent,
         "traj_sdxl_hires_latent": g_traj_sdxl_hires_latent}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", nargs="*")
    a = ap.parse_args()
    for name, fn in CASES.items():
        if a.only and name not in a.only:
            continue
        fn()


if __name__ == "__main__":
    main()
