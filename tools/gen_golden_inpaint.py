"""ORACLE tooling for the inpainting path - writes tests/golden/{inpaint_unet_*,traj_inpaint_ddim}.npz from the reference's own
modules (the 9-channel UNetModel of inpainting.yaml, LatentInpaintDiffusion with hybrid conditioning, DDIMSampler.sample with
eta = 1), on the name-keyed synthetic weights and `synth_input` tensors of oracle/gen_golden.py, whose import stubs and helpers it
reuses (that module is imported, not changed).  Only the .npz files are committed; a rerun reproduces them exactly.

    python tools/gen_golden_inpaint.py [--only NAME ...] [--skip-full]
"""
import argparse
import contextlib
import hashlib
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from oracle import gen_golden as G  # noqa: E402  (installs the import stubs and puts the reference on sys.path)
from oracle.gen_golden import SEED, fp32_forward, save, synth_fill_, synth_input  # noqa: E402

INPAINT = lambda cfg: dict(cfg, in_channels=9)  # noqa: E731  (inpainting.yaml: 4 latent + 1 mask + 4 masked-image channels)


def _key_digest(module):
    items = sorted(f"{k}:{tuple(v.shape)}" for k, v in module.state_dict().items())
    return hashlib.sha1("\n".join(items).encode()).hexdigest(), len(items)


def _unet_case(name, cfg, B, L, mctx, tvals):
    m = G.R_unet.UNetModel(**cfg)
    synth_fill_(m, SEED, prefix="unet.")
    x = synth_input(name + ".x", (B, 9, L, L), SEED)
    ctx = synth_input(name + ".ctx", (B, mctx, cfg["context_dim"]), SEED)
    t = torch.tensor(tvals, dtype=torch.float32)
    t0 = time.time()
    with fp32_forward():
        y = m(x, timesteps=t, context=ctx)
    dt = time.time() - t0
    sha, n = _key_digest(m)
    save(name, dict(cfg=cfg, B=B, L=L, m=mctx, seed=SEED, prefix="unet.", n_params=sum(p.numel() for p in m.parameters()),
                    n_keys=n, keys_sha1=sha, conv_in_shape=list(m.input_blocks[0][0].weight.shape), ref_cpu_seconds=dt,
                    threads=torch.get_num_threads()), t=t, y=y)


def g_inpaint_unet_tiny():
    _unet_case("inpaint_unet_tiny", INPAINT(G.TINY_UNET), 2, 16, 77, [10.0, 731.25])


def g_inpaint_unet_small_sd():
    _unet_case("inpaint_unet_small_sd", INPAINT(G.SMALL_SD_UNET), 2, 16, 77, [3.5, 900.0])


def g_inpaint_unet_sd15_full():
    # the SD1.5 inpainting UNet (inpainting.yaml unet_config), B=2 (one image x CFG), L=64
    _unet_case("inpaint_unet_sd15_full", INPAINT(G.SD15_UNET), 2, 64, 77, [981.5, 981.5])


def _tiny_inpaint_ldm():
    from ldm.models.diffusion.ddpm import LatentInpaintDiffusion
    ldm = LatentInpaintDiffusion(first_stage_config={"target": "ldm.models.autoencoder.AutoencoderKL",
                                                     "params": dict(ddconfig=G.TINY_DD, lossconfig={"target": "torch.nn.Identity"},
                                                                    embed_dim=4)},
                                 cond_stage_config={"target": "torch.nn.Identity"},
                                 unet_config={"target": "ldm.modules.diffusionmodules.openaimodel.UNetModel",
                                              "params": INPAINT(G.TINY_UNET)},
                                 linear_start=0.00085, linear_end=0.012, timesteps=1000, conditioning_key="hybrid",
                                 scale_factor=0.18215, use_ema=False, cond_stage_trainable=False, first_stage_key="jpg",
                                 cond_stage_key="txt", image_size=16, channels=4)
    synth_fill_(ldm.model.diffusion_model, SEED, prefix="unet.")
    synth_fill_(ldm.first_stage_model, SEED, prefix="vae.")
    return ldm.eval()


TRAJ = dict(B=2, L=16, HW=32, S=10, eta=1.0, cfg=7.5, mask_threshold=0.3)


def traj_inputs(B, L, HW, seed, mask_threshold):
    """The trajectory's inputs, by synth_input name (the GPU tests rebuild them with this same function's recipe)."""
    return dict(c=synth_input("inpaint.c", (B, 77, 96), seed), uc=synth_input("inpaint.uc", (B, 77, 96), seed),
                image=synth_input("inpaint.img", (B, 3, HW, HW), seed, 0.5).clamp(-1, 1),
                mask=(synth_input("inpaint.mask", (B, 1, HW, HW), seed) > mask_threshold).float(),
                enc_noise=synth_input("inpaint.encnoise", (B, 4, L, L), seed))


def g_traj_inpaint_ddim():
    """inpaint.py:160-281 on a tiny LatentInpaintDiffusion through the reference's DDIMSampler.sample (eta 1.0, CFG 7.5, S 10): the
    c_concat of :218-227 (nearest-downsampled mask, first-stage encoding of the masked image with injected posterior noise), one
    c_cat object in both dicts (:244-245), the start code of np.random.RandomState(seed) (:166-169), per-step noise injected through
    ddim.noise_like, then decode_first_stage."""
    import ldm.models.diffusion.ddim as R_ddim
    from ldm.models.diffusion.ddim import DDIMSampler
    ldm = _tiny_inpaint_ldm()
    B, L, HW, S = TRAJ["B"], TRAJ["L"], TRAJ["HW"], TRAJ["S"]
    inp = traj_inputs(B, L, HW, SEED, TRAJ["mask_threshold"])
    R_ddim.tqdm = lambda it, **k: it
    calls = []

    def noise_like(shape, device, repeat=False):
        assert not repeat
        z = synth_input(f"inpaint.noise{len(calls)}", tuple(shape), SEED)
        calls.append(len(calls))
        return z
    orig_noise_like = R_ddim.noise_like
    R_ddim.noise_like = noise_like
    dd = DDIMSampler(ldm)
    dd.register_buffer = lambda name, attr: setattr(dd, name, attr)  # keep the fp32 tables on the CPU (see gen_golden.g_schedules)
    try:
        with fp32_forward(), contextlib.redirect_stdout(open(os.devnull, "w")):
            fsm = ldm.first_stage_model
            masked = inp["image"] * (inp["mask"] < 0.5)
            # AutoencoderKL.encode (autoencoder.py:324-331) minus its unconditional x.half(), then get_first_stage_encoding (ddpm.py:575-582)
            post = G.DiagonalGaussianDistribution(fsm.quant_conv(fsm.encoder(masked)))
            z_masked = 0.18215 * (post.mean + post.std * inp["enc_noise"])
            c_cat = torch.cat([torch.nn.functional.interpolate(inp["mask"], size=(L, L)), z_masked], dim=1)
            cond = {"c_concat": [c_cat], "c_crossattn": [inp["c"]]}
            uc_full = {"c_concat": [c_cat], "c_crossattn": [inp["uc"]]}
            start = torch.from_numpy(np.random.RandomState(SEED).randn(B, 4, L, L)).to(torch.float32)
            x, _ = dd.sample(S, B, [4, L, L], cond, verbose=False, eta=TRAJ["eta"], unconditional_guidance_scale=TRAJ["cfg"],
                             unconditional_conditioning=uc_full, x_T=start)
            img = ldm.decode_first_stage(x)
    finally:
        R_ddim.noise_like = orig_noise_like
    assert len(calls) == S
    save("traj_inpaint_ddim", dict(TRAJ, seed=SEED, unet=INPAINT(G.TINY_UNET), dd=G.TINY_DD),
         c_cat=c_cat, start=start, ddim_sigmas=torch.as_tensor(np.asarray(dd.ddim_sigmas)), x=x, img=img)


CASES = {"inpaint_unet_tiny": g_inpaint_unet_tiny, "inpaint_unet_small_sd": g_inpaint_unet_small_sd,
         "inpaint_unet_sd15_full": g_inpaint_unet_sd15_full, "traj_inpaint_ddim": g_traj_inpaint_ddim}


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
