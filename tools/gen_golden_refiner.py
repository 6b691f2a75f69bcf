"""ORACLE tooling for the SDXL refiner stage and DPM++ 2M sampling - writes tests/golden/{sgm_refiner_unet_*, traj_sdxl_dpmpp2m,
traj_sdxl_refiner, sdxl_sampler_toy}.npz from the reference's own modules (sgm UNetModel at the sd_xl_refiner.yaml settings,
DPMPP2MSampler, Img2Img- / Txt2NoisyDiscretizationWrapper, DiscreteDenoiser with EpsScaling, VanillaCFG, OpenAIWrapper), on the
name-keyed synthetic weights and `synth_input` tensors of oracle/gen_golden.py, whose import stubs and helpers it reuses (that
module is imported, not changed).  Only the .npz files are committed; a rerun reproduces them exactly (apart from timing meta).

    python tools/gen_golden_refiner.py [--only NAME ...] [--skip-full]
"""
import argparse
import contextlib
import hashlib
import os
import sys
import time
import types

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from oracle import gen_golden as G  # noqa: E402  (installs the import stubs and puts the reference on sys.path)
from oracle.gen_golden import SEED, fp32_forward, save, synth_fill_, synth_input  # noqa: E402

REF_YAML = os.path.join(G.REF, "sdxl", "configs", "inference", "sd_xl_refiner.yaml")
# sd_xl_refiner.yaml network params (use_checkpoint only selects activation checkpointing for training: off for the CPU forward)
REFINER_UNET = dict(adm_in_channels=2560, num_classes="sequential", use_checkpoint=False, in_channels=4, out_channels=4, model_channels=384,
                    attention_resolutions=[4, 2], num_res_blocks=2, channel_mult=[1, 2, 4, 4], num_head_channels=64,
                    use_linear_in_transformer=True, transformer_depth=4, context_dim=[1280, 1280, 1280, 1280],
                    spatial_transformer_attn_type="softmax-xformers")
# the refiner's structure at small widths: four levels, attention on the middle two only, int depth, list-valued context_dim
TINY_REFINER_UNET = dict(adm_in_channels=96, num_classes="sequential", use_checkpoint=False, in_channels=4, out_channels=4, model_channels=64,
                         attention_resolutions=[4, 2], num_res_blocks=2, channel_mult=[1, 2, 4, 4], num_head_channels=32,
                         use_linear_in_transformer=True, transformer_depth=2, context_dim=[96, 96],
                         spatial_transformer_attn_type="softmax-xformers")
REFINER_SEED = SEED + 1  # the tiny refiner of the two-stage trajectory: weights independent of the tiny base's
LEGACY = {"target": "sgm.modules.diffusionmodules.discretizer.LegacyDDPMDiscretization"}


def _key_digest(module):
    items = sorted(f"{k}:{tuple(v.shape)}" for k, v in module.state_dict().items())
    return hashlib.sha1("\n".join(items).encode()).hexdigest(), len(items)


def _ref_yaml_network_params():
    import yaml
    return yaml.safe_load(open(REF_YAML))["model"]["params"]["network_config"]["params"]


def _unet_case(name, cfg, B, L, mctx, tvals, extra=None):
    SU = G._import_sgm()[0]
    m = SU.UNetModel(**cfg)
    synth_fill_(m, SEED, prefix="sgm_unet.")
    cdim = cfg["context_dim"][0] if isinstance(cfg["context_dim"], list) else cfg["context_dim"]
    x = synth_input(name + ".x", (B, 4, L, L), SEED)
    ctx = synth_input(name + ".ctx", (B, mctx, cdim), SEED)
    y = synth_input(name + ".y", (B, cfg["adm_in_channels"]), SEED)
    t = torch.tensor(tvals, dtype=torch.float32)
    t0 = time.time()
    with fp32_forward():
        out = m(x, timesteps=t, context=ctx, y=y)
    dt = time.time() - t0
    sha, n = _key_digest(m)
    meta = dict(cfg=cfg, B=B, L=L, m=mctx, ctx_dim=cdim, seed=SEED, prefix="sgm_unet.", n_params=sum(p.numel() for p in m.parameters()),
                n_keys=n, keys_sha1=sha, ref_cpu_seconds=dt, threads=torch.get_num_threads())
    meta.update(extra or {})
    save(name, meta, t=t, y=out)


def g_refiner_unet_tiny():
    _unet_case("sgm_refiner_unet_tiny", TINY_REFINER_UNET, 2, 16, 77, [3.0, 180.0])


def g_refiner_unet_small():
    _unet_case("sgm_refiner_unet_small", REFINER_UNET, 2, 32, 77, [20.0, 150.0])


def g_refiner_unet_full():
    # the full refiner at a 1024^2 image (L = 128), B = 2 (one image x CFG), timesteps in the refiner's range (strength <= 0.2: t < 200)
    _unet_case("sgm_refiner_unet_full", REFINER_UNET, 2, 128, 77, [150.0, 37.0], extra=dict(yaml_network_params=_ref_yaml_network_params()))


def _sgm():
    SU, DN, DZ, GD, SM, WR = G._import_sgm()
    SM.denoising_status_queue = types.SimpleNamespace(put=lambda *a, **k: None)
    from scripts.demo.discretization import Img2ImgDiscretizationWrapper, Txt2NoisyDiscretizationWrapper
    return SU, DN, SM, WR, Img2ImgDiscretizationWrapper, Txt2NoisyDiscretizationWrapper


def _denoiser(DN):
    return DN.DiscreteDenoiser(scaling_config={"target": "sgm.modules.diffusionmodules.denoiser_scaling.EpsScaling"}, num_idx=1000,
                               discretization_config=LEGACY)


def _dpm(SM, steps, cfg):
    return SM.DPMPP2MSampler(discretization_config=LEGACY, num_steps=steps, verbose=False, device="cpu",
                             guider_config={"target": "sgm.modules.diffusionmodules.guiders.VanillaCFG", "params": {"scale": cfg}})


def _cond(tag, B, cdim, vdim):
    return ({"crossattn": synth_input(tag + ".c", (B, 77, cdim), SEED), "vector": synth_input(tag + ".cv", (B, vdim), SEED)},
            {"crossattn": synth_input(tag + ".uc", (B, 77, cdim), SEED), "vector": synth_input(tag + ".ucv", (B, vdim), SEED)})


DPM_TRAJ = dict(B=2, L=16, S=6, cfg=5.0)


def g_traj_sdxl_dpmpp2m():
    """6 DPMPP2MSampler steps (DiscreteDenoiser + EpsScaling + VanillaCFG 5) on the tiny sgm UNet, then the tiny first stage's
    decode with scale_factor 0.13025 (do_sample, sdxl_image_generator_utils.py:695-734, with the default SDXL sampler)."""
    SU, DN, SM, WR, _, _ = _sgm()
    unet = synth_fill_(SU.UNetModel(**G.TINY_SGM_UNET), SEED, prefix="sgm_unet.")
    model, den = WR.OpenAIWrapper(unet), _denoiser(DN)
    B, L, S = DPM_TRAJ["B"], DPM_TRAJ["L"], DPM_TRAJ["S"]
    smp = _dpm(SM, S, DPM_TRAJ["cfg"])
    c, uc = _cond("dpm2m", B, 128, 96)
    x0 = synth_input("dpm2m.x0", (B, 4, L, L), SEED)
    ae = G._make_ae(G.TINY_DD)
    with fp32_forward(), contextlib.redirect_stdout(open(os.devnull, "w")):
        x = smp(lambda inp, sigma, cc: den(model, inp, sigma, cc), x0.clone(), cond=c, uc=uc)
        img = ae.decode(x / 0.13025)
    save("traj_sdxl_dpmpp2m", dict(DPM_TRAJ, seed=SEED, unet=G.TINY_SGM_UNET, dd=G.TINY_DD, scale_factor=0.13025),
         sigmas=smp.discretization(S), x=x, img=img)


REF_TRAJ = dict(B=2, L=16, S=10, strength=0.3, cfg=5.0)


def g_traj_sdxl_refiner():
    """The two-stage run of sdxl_use_refiner on tiny nets: the base samples with Txt2NoisyDiscretizationWrapper(strength,
    original_steps = S) (init_sampling :404-407), then apply_refiner -> do_img2img(skip_encode, add_noise = False) with an
    Img2ImgDiscretizationWrapper(strength) sampler on the refiner (sdxl_image_generator.py:307-347, :555-635;
    sdxl_image_generator_utils.py:986-1016), DPM++ 2M in both stages, the shared first stage decodes."""
    SU, DN, SM, WR, I2I, T2N = _sgm()
    base = synth_fill_(SU.UNetModel(**G.TINY_SGM_UNET), SEED, prefix="sgm_unet.")
    refiner = synth_fill_(SU.UNetModel(**TINY_REFINER_UNET), REFINER_SEED, prefix="sgm_unet.")
    B, L, S, k, cfg = REF_TRAJ["B"], REF_TRAJ["L"], REF_TRAJ["S"], REF_TRAJ["strength"], REF_TRAJ["cfg"]
    c, uc = _cond("refb", B, 128, 96)
    c2, uc2 = _cond("refr", B, 96, 96)
    x0 = synth_input("refb.x0", (B, 4, L, L), SEED)
    ae = G._make_ae(G.TINY_DD)
    s1 = _dpm(SM, S, cfg)
    s1.discretization = T2N(s1.discretization, strength=k, original_steps=S)
    s2 = _dpm(SM, S, cfg)
    s2.discretization = I2I(s2.discretization, strength=k)
    m1, d1 = WR.OpenAIWrapper(base), _denoiser(DN)
    m2, d2 = WR.OpenAIWrapper(refiner), _denoiser(DN)
    with fp32_forward(), contextlib.redirect_stdout(open(os.devnull, "w")):
        z = s1(lambda inp, sigma, cc: d1(m1, inp, sigma, cc), x0.clone(), cond=c, uc=uc)
        sig2 = s2.discretization(s2.num_steps)
        noised_z = z / torch.sqrt(1.0 + sig2[0] ** 2.0)
        x = s2(lambda inp, sigma, cc: d2(m2, inp, sigma, cc), noised_z, cond=c2, uc=uc2)
        img = ae.decode(x / 0.13025)
    save("traj_sdxl_refiner", dict(REF_TRAJ, seed=SEED, refiner_seed=REFINER_SEED, unet=G.TINY_SGM_UNET, refiner_unet=TINY_REFINER_UNET,
                                   dd=G.TINY_DD, scale_factor=0.13025),
         sigmas_base=s1.discretization(S), sigmas_refiner=sig2, z=z, x=x, img=img)


TOY_STEPS = [5, 20, 30, 50]
TOY_STRENGTHS = [0.0, 0.15, 0.3, 0.5, 1.0]
TOY_I2I_FOR_COMPOSED = 0.6  # the Img2Img strength of the composed (img2img base stage) schedules
TOY = dict(B=2, L=8, cfg=5.0, txt2img_steps=20, stage_steps=30, stage_strength=0.15)


def toy_denoiser(inp, sigma, c):
    """Analytic stand-in for DiscreteDenoiser(network, ...) - restated in tests/test_refiner_cpu.py: depends on the input, the
    per-sample sigma and the (batch-doubled) conditioning vector, so the guidance and both multistep branches are exercised."""
    s = sigma.reshape(-1, 1, 1, 1)
    return inp / (1.0 + s ** 2) + c["vector"].reshape(-1, 4, 1, 1) * (s / (1.0 + s))


def _tag(steps, strength):
    return f"{steps}_{int(round(strength * 100)):03d}"


def _mult_table(smp, sigmas):
    """get_variables / get_mult of the reference for every step of a run over `sigmas` (s_in of batch 1): [n - 1, 4] fp32, NaN where
    the first step has no m3 / m4."""
    s_in = torch.ones([1])
    rows = []
    for i in range(len(sigmas) - 1):
        prev = None if i == 0 else s_in * sigmas[i - 1]
        h, r, t, t_next = smp.get_variables(s_in * sigmas[i], s_in * sigmas[i + 1], prev)
        m = [v.reshape(()) for v in smp.get_mult(h, r, t, t_next, prev)]
        rows.append(torch.stack(m + [torch.tensor(float("nan"))] * (4 - len(m))))
    return torch.stack(rows) if rows else torch.zeros((0, 4))


def g_sdxl_sampler_toy():
    """Schedules of both discretization wrappers and of the composed pair, the DPM++ 2M multiplier tables over them, and DPM++ 2M
    trajectories of the reference's sampler under toy_denoiser (txt2img, the pruned base stage, the refiner stage)."""
    SU, DN, SM, WR, I2I, T2N = _sgm()
    from sgm.modules.diffusionmodules.discretizer import LegacyDDPMDiscretization
    arrays = {}
    for steps in TOY_STEPS:
        smp = _dpm(SM, steps, TOY["cfg"])
        plain = LegacyDDPMDiscretization()(steps)
        arrays[f"plain_{steps}"] = plain
        arrays[f"m_plain_{steps}"] = _mult_table(smp, plain)
        for k in TOY_STRENGTHS:
            t2n = T2N(LegacyDDPMDiscretization(), strength=k, original_steps=steps)(steps)
            i2i = I2I(LegacyDDPMDiscretization(), strength=k)(steps)
            comp = T2N(I2I(LegacyDDPMDiscretization(), strength=TOY_I2I_FOR_COMPOSED), strength=k, original_steps=steps)(steps)
            for nm, sg in (("t2n", t2n), ("i2i", i2i), ("comp", comp)):
                arrays[f"{nm}_{_tag(steps, k)}"] = sg
                arrays[f"m_{nm}_{_tag(steps, k)}"] = _mult_table(smp, sg)
    B, L, cfg = TOY["B"], TOY["L"], TOY["cfg"]
    c = {"vector": synth_input("toy.cv", (B, 4), SEED)}
    uc = {"vector": synth_input("toy.ucv", (B, 4), SEED)}
    x0 = synth_input("toy.x0", (B, 4, L, L), SEED)
    with torch.no_grad():
        s = _dpm(SM, TOY["txt2img_steps"], cfg)
        arrays["traj_txt2img"] = s(toy_denoiser, x0.clone(), cond=c, uc=uc)
        s = _dpm(SM, TOY["stage_steps"], cfg)
        s.discretization = T2N(s.discretization, strength=TOY["stage_strength"], original_steps=TOY["stage_steps"])
        z = s(toy_denoiser, x0.clone(), cond=c, uc=uc)
        arrays["traj_base"] = z
        s = _dpm(SM, TOY["stage_steps"], cfg)
        s.discretization = I2I(s.discretization, strength=TOY["stage_strength"])
        sig = s.discretization(s.num_steps)
        arrays["traj_refiner"] = s(toy_denoiser, z / torch.sqrt(1.0 + sig[0] ** 2.0), cond=c, uc=uc)
    save("sdxl_sampler_toy", dict(TOY, seed=SEED, steps=TOY_STEPS, strengths=TOY_STRENGTHS, i2i_for_composed=TOY_I2I_FOR_COMPOSED),
         x0=x0, **arrays)


CASES = {"sgm_refiner_unet_tiny": g_refiner_unet_tiny, "sgm_refiner_unet_small": g_refiner_unet_small,
         "sgm_refiner_unet_full": g_refiner_unet_full, "traj_sdxl_dpmpp2m": g_traj_sdxl_dpmpp2m, "traj_sdxl_refiner": g_traj_sdxl_refiner,
         "sdxl_sampler_toy": g_sdxl_sampler_toy}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", nargs="*")
    ap.add_argument("--skip-full", action="store_true")
    a = ap.parse_args()
    torch.manual_seed(0)
    for name, fn in CASES.items():
        if a.only and name not in a.only:
            continue
        if a.skip_full and name.endswith("_full"):
            continue
        fn()


if __name__ == "__main__":
    main()
