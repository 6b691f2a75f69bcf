"""ORACLE tooling for the rest of Cremage's SDXL sampler menu - writes tests/golden/{sdxl_samplers_sched, sdxl_samplers_toy,
traj_sdxl_heun_edm, traj_sdxl_euler_ancestral, traj_sdxl_dpmpp2s_ancestral, traj_sdxl_linear_multistep, traj_sdxl_samplers_extra}.npz
from the reference's own modules (EDMDiscretization, HeunEDMSampler, EulerAncestralSampler, DPMPP2SAncestralSampler,
LinearMultistepSampler and DPMPP2MSampler with their sampling_utils, Img2Img- / Txt2NoisyDiscretizationWrapper, DiscreteDenoiser with
EpsScaling, VanillaCFG, OpenAIWrapper and the sgm UNetModel), on the name-keyed synthetic weights and `synth_input` tensors of
oracle/gen_golden.py, whose import stubs and helpers it reuses (that module is imported, not changed).  Every torch.randn_like the
samplers make returns the next recorded tensor `synth_input(f"{tag}.noise{k}")` instead (as oracle/gen_golden.py does for Euler-a),
and the count of draws is stored.  Only the .npz files are committed; a rerun reproduces the arrays exactly.

    python tools/gen_golden_sdxl_samplers.py [--only NAME ...]
"""
import argparse
import contextlib
import os
import sys
import types

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from oracle import gen_golden as G  # noqa: E402  (installs the import stubs and puts the reference on sys.path)
from oracle.gen_golden import SEED, fp32_forward, save, synth_fill_, synth_input  # noqa: E402

LEGACY = {"target": "sgm.modules.diffusionmodules.discretizer.LegacyDDPMDiscretization"}
EDM_PARAMS = {"sigma_min": 0.0292, "sigma_max": 14.6146, "rho": 3.0}  # Cremage's preferences (preferences.py:149-151)
EDM = {"target": "sgm.modules.diffusionmodules.discretizer.EDMDiscretization", "params": EDM_PARAMS}
DISC = {"legacy": LEGACY, "edm": EDM}
CLASSES = {"euler_edm": "EulerEDMSampler", "heun_edm": "HeunEDMSampler", "euler_ancestral": "EulerAncestralSampler",
           "dpmpp2s_ancestral": "DPMPP2SAncestralSampler", "dpmpp2m": "DPMPP2MSampler", "linear_multistep": "LinearMultistepSampler"}
# get_sampler's arguments with Cremage's default preferences (sdxl_image_generator_utils.py:451-522, preferences.py:159-165)
DEFAULTS = {"euler_edm": dict(s_churn=0.0, s_tmin=0.0, s_tmax=999.0, s_noise=1.0), "heun_edm": dict(s_churn=0.0, s_tmin=0.0, s_tmax=999.0, s_noise=1.0),
            "euler_ancestral": dict(eta=1.0, s_noise=1.0), "dpmpp2s_ancestral": dict(eta=1.0, s_noise=1.0), "dpmpp2m": {},
            "linear_multistep": dict(order=4)}
NEW = ["heun_edm", "euler_ancestral", "dpmpp2s_ancestral", "linear_multistep"]


def _sgm():
    SU, DN, DZ, GD, SM, WR = G._import_sgm()
    SM.denoising_status_queue = types.SimpleNamespace(put=lambda *a, **k: None)
    from scripts.demo.discretization import Img2ImgDiscretizationWrapper, Txt2NoisyDiscretizationWrapper
    return SU, DN, DZ, SM, WR, Img2ImgDiscretizationWrapper, Txt2NoisyDiscretizationWrapper


def _denoiser(DN):
    return DN.DiscreteDenoiser(scaling_config={"target": "sgm.modules.diffusionmodules.denoiser_scaling.EpsScaling"}, num_idx=1000,
                               discretization_config=LEGACY)


def make(SM, key, disc, steps, cfg, **over):
    return getattr(SM, CLASSES[key])(discretization_config=DISC[disc], num_steps=steps, verbose=False, device="cpu",
                                     guider_config={"target": "sgm.modules.diffusionmodules.guiders.VanillaCFG", "params": {"scale": cfg}},
                                     **dict(DEFAULTS[key], **over))


@contextlib.contextmanager
def recorded_noise(tag):
    """torch.randn_like(x) -> synth_input(f"{tag}.noise{k}", x.shape) for the k-th draw; yields the list of drawn shapes."""
    draws, orig = [], torch.randn_like

    def fake(x, **kw):
        z = synth_input(f"{tag}.noise{len(draws)}", tuple(x.shape), SEED).to(device=x.device, dtype=x.dtype)
        draws.append(tuple(x.shape))
        return z
    torch.randn_like = fake
    try:
        yield draws
    finally:
        torch.randn_like = orig


def toy_denoiser(inp, sigma, c):
    """Analytic stand-in for DiscreteDenoiser(network, ...) (the one of tools/gen_golden_refiner.py) - restated in
    tests/test_sdxl_samplers_cpu.py."""
    s = sigma.reshape(-1, 1, 1, 1)
    return inp / (1.0 + s ** 2) + c["vector"].reshape(-1, 4, 1, 1) * (s / (1.0 + s))


SCHED_STEPS = [5, 20, 30, 50]
SCHED_STRENGTH = 0.3   # Img2Img (C5's face-fix strength) and Txt2Noisy (a refined base stage) wrappers of the EDM schedule
TABLE_STEPS = 30


def _lms_table(SU_, sigmas, order):
    t = sigmas.numpy()
    out = np.full((len(t) - 1, order), np.nan, dtype=np.float64)
    for i in range(len(t) - 1):
        cur = min(i + 1, order)
        out[i, :cur] = [SU_.linear_multistep_coeff(cur, t, i, j) for j in range(cur)]
    return out


def g_sdxl_samplers_sched():
    """EDM sigmas (alone and wrapped), and per schedule the ancestral steps, DPM++ 2S's multipliers and midpoint sigmas and the LMS
    coefficients of the reference's own functions, over [b = 2] vectors as its samplers form them."""
    SU, DN, DZ, SM, WR, I2I, T2N = _sgm()
    from sgm.modules.diffusionmodules import sampling_utils as SUT
    arrays = {}
    for n in SCHED_STEPS:
        arrays[f"edm_{n}"] = DZ.EDMDiscretization(**EDM_PARAMS)(n)
        arrays[f"edm_i2i_{n}"] = I2I(DZ.EDMDiscretization(**EDM_PARAMS), strength=SCHED_STRENGTH)(n)
        arrays[f"edm_t2n_{n}"] = T2N(DZ.EDMDiscretization(**EDM_PARAMS), strength=SCHED_STRENGTH, original_steps=n)(n)
    arrays["edm_default_20"] = DZ.EDMDiscretization()(20)   # the class defaults (0.002, 80, 7)
    s_in = torch.ones([2])
    dpm = make(SM, "dpmpp2s_ancestral", "edm", TABLE_STEPS, 5.0)
    for name, sig in (("legacy", DZ.LegacyDDPMDiscretization()(TABLE_STEPS)), ("edm", arrays[f"edm_{TABLE_STEPS}"]),
                      ("edm_t2n", arrays[f"edm_t2n_{TABLE_STEPS}"])):
        for eta in (1.0, 0.5):
            tag = f"{name}_eta{int(eta * 10):02d}"
            down, up, m, mid = [], [], [], []
            for i in range(len(sig) - 1):
                d, u = SUT.get_ancestral_step(s_in * sig[i], s_in * sig[i + 1], eta=eta)
                down.append(d[0]), up.append(u[0])
                if torch.sum(d) < 1e-14:
                    m.append(torch.full((4,), float("nan"))), mid.append(torch.tensor(float("nan")))
                    continue
                h, s, t, t_next = dpm.get_variables(s_in * sig[i], d)
                m.append(torch.stack([v[0] for v in dpm.get_mult(h, s, t, t_next)]))
                mid.append(SUT.to_sigma(s)[0])
            arrays[f"down_{tag}"], arrays[f"up_{tag}"] = torch.stack(down), torch.stack(up)
            arrays[f"m_{tag}"], arrays[f"mid_{tag}"] = torch.stack(m), torch.stack(mid)
        arrays[f"lms_{name}"] = _lms_table(SUT, sig, 4)
        arrays[f"sigmas_{name}"] = sig
    save("sdxl_samplers_sched", dict(steps=SCHED_STEPS, strength=SCHED_STRENGTH, edm=EDM_PARAMS, table_steps=TABLE_STEPS, b=2), **arrays)


TOY = dict(B=2, L=8, cfg=5.0, steps=12)
# name -> (sampler key, schedule, option overrides, wrapper): every sampler on both schedules, then the options and wrappers
TOY_CASES = {f"{k}_{d}": (k, d, {}, None) for k in CLASSES for d in ("legacy", "edm")}
TOY_CASES.update({
    "heun_edm_churn_legacy": ("heun_edm", "legacy", dict(s_churn=1.0, s_tmin=0.5, s_tmax=10.0, s_noise=0.9), None),
    "heun_edm_churn_edm": ("heun_edm", "edm", dict(s_churn=2.0, s_noise=1.1), None),
    "euler_edm_churn_edm": ("euler_edm", "edm", dict(s_churn=1.0), None),
    "euler_ancestral_eta_edm": ("euler_ancestral", "edm", dict(eta=0.5, s_noise=0.8), None),
    "dpmpp2s_ancestral_eta_legacy": ("dpmpp2s_ancestral", "legacy", dict(eta=0.5, s_noise=0.8), None),
    "linear_multistep_o2_edm": ("linear_multistep", "edm", dict(order=2), None),
    "linear_multistep_o6_legacy": ("linear_multistep", "legacy", dict(order=6), None),
    "heun_edm_t2n_edm": ("heun_edm", "edm", {}, ("t2n", 0.3)),
    "dpmpp2s_ancestral_t2n_legacy": ("dpmpp2s_ancestral", "legacy", {}, ("t2n", 0.3)),
    "euler_ancestral_i2i_edm": ("euler_ancestral", "edm", {}, ("i2i", 0.5)),
    "linear_multistep_i2i_legacy": ("linear_multistep", "legacy", {}, ("i2i", 0.5)),
})


def _wrap(smp, wrapper, steps, I2I, T2N):
    if wrapper is None:
        return
    kind, k = wrapper
    smp.discretization = I2I(smp.discretization, strength=k) if kind == "i2i" else T2N(smp.discretization, strength=k, original_steps=steps)


def g_sdxl_samplers_toy():
    """Every sampler's loop under toy_denoiser: the final latents, the evaluation sigmas in call order, their snapped indices
    (DiscreteDenoiser.sigma_to_idx) and the number of noise draws."""
    SU, DN, DZ, SM, WR, I2I, T2N = _sgm()
    den = _denoiser(DN)
    B, L, cfg, steps = TOY["B"], TOY["L"], TOY["cfg"], TOY["steps"]
    c = {"vector": synth_input("toy.cv", (B, 4), SEED)}
    uc = {"vector": synth_input("toy.ucv", (B, 4), SEED)}
    x0 = synth_input("toy.x0", (B, 4, L, L), SEED)
    arrays, draws = {}, {}
    for name, (key, disc, over, wrapper) in TOY_CASES.items():
        smp = make(SM, key, disc, steps, cfg, **over)
        _wrap(smp, wrapper, steps, I2I, T2N)
        ev = []

        def rec(inp, sigma, cc):
            ev.append(sigma[0].clone())   # the batch-doubled sigma: every entry is the same
            return toy_denoiser(inp, sigma, cc)
        with torch.no_grad(), recorded_noise("toy." + name) as dr, contextlib.redirect_stdout(open(os.devnull, "w")):
            arrays["x_" + name] = smp(rec, x0.clone(), cond=c, uc=uc)
        ev = torch.stack(ev)
        arrays["ev_" + name] = ev
        arrays["idx_" + name] = den.sigma_to_idx(ev)
        draws[name] = len(dr)
    save("sdxl_samplers_toy", dict(TOY, seed=SEED, cases={k: [v[0], v[1], v[2], v[3]] for k, v in TOY_CASES.items()}, draws=draws),
         x0=x0, **arrays)


TRAJ = dict(B=2, L=16, S=6, cfg=5.0)


def _cond(tag, B):
    return ({"crossattn": synth_input(tag + ".c", (B, 77, 128), SEED), "vector": synth_input(tag + ".cv", (B, 96), SEED)},
            {"crossattn": synth_input(tag + ".uc", (B, 77, 128), SEED), "vector": synth_input(tag + ".ucv", (B, 96), SEED)})


def _tiny():
    SU, DN, DZ, SM, WR, I2I, T2N = _sgm()
    unet = synth_fill_(SU.UNetModel(**G.TINY_SGM_UNET), SEED, prefix="sgm_unet.")
    model, den = WR.OpenAIWrapper(unet), _denoiser(DN)
    return SM, I2I, T2N, (lambda inp, sigma, cc: den(model, inp, sigma, cc)), G._make_ae(G.TINY_DD)


def _traj(SM, fn, key, disc, tag, steps=None, over=None, wrapper=None, I2I=None, T2N=None, x_in=None, decode=True, ae=None):
    B, L, S, cfg = TRAJ["B"], TRAJ["L"], steps or TRAJ["S"], TRAJ["cfg"]
    smp = make(SM, key, disc, S, cfg, **(over or {}))
    _wrap(smp, wrapper, S, I2I, T2N)
    c, uc = _cond(tag, B)
    x0 = synth_input(tag + ".x0", (B, 4, L, L), SEED) if x_in is None else x_in
    with fp32_forward(), recorded_noise(tag) as dr, contextlib.redirect_stdout(open(os.devnull, "w")):
        x = smp(fn, x0.clone(), cond=c, uc=uc)
        img = ae.decode(x / 0.13025) if decode else None
    return smp, x, img, len(dr)


def _g_traj(key):
    """TRAJ["S"] steps of `key` on the tiny sgm UNet (DiscreteDenoiser + EpsScaling + VanillaCFG 5) on both schedules with recorded
    noise, and the tiny first stage's decode (do_sample, sdxl_image_generator_utils.py:695-734)."""
    SM, I2I, T2N, fn, ae = _tiny()
    arrays, meta = {}, dict(TRAJ, key=key, seed=SEED, unet=G.TINY_SGM_UNET, dd=G.TINY_DD, scale_factor=0.13025, edm=EDM_PARAMS,
                            options=DEFAULTS[key], draws={})
    for disc in ("legacy", "edm"):
        tag = f"{key}.{disc}"
        smp, x, img, nd = _traj(SM, fn, key, disc, tag, ae=ae)
        arrays[f"sigmas_{disc}"], arrays[f"x_{disc}"], arrays[f"img_{disc}"] = smp.discretization(TRAJ["S"]), x, img
        meta["draws"][disc] = nd
    if key == "heun_edm":
        meta["churn"] = dict(s_churn=1.0, s_noise=0.9)
        _, x, _, nd = _traj(SM, fn, key, "legacy", f"{key}.churn", over=meta["churn"], decode=False)
        arrays["x_churn"] = x
        meta["draws"]["churn"] = nd
    save(f"traj_sdxl_{key}", meta, **arrays)


EXTRA = dict(i2i_steps=20, i2i_strength=0.3, t2n_steps=10, t2n_strength=0.3)


def g_traj_sdxl_samplers_extra():
    """DPM++ 2M on the EDM schedule; an img2img with DPM++ 2S ancestral on the EDM schedule (do_img2img, the face-fix re-entry of
    BASELINE config 5, strength 0.3; oracle/gen_golden.py g_sgm_img2img's encode and noising); and a Txt2Noisy-pruned base stage
    with HeunEDM on the EDM schedule, whose last step makes two calls (its last sigma is not 0)."""
    SM, I2I, T2N, fn, ae = _tiny()
    from ldm.modules.distributions.distributions import DiagonalGaussianDistribution
    meta = dict(TRAJ, **EXTRA, seed=SEED, unet=G.TINY_SGM_UNET, dd=G.TINY_DD, scale_factor=0.13025, edm=EDM_PARAMS, draws={})
    arrays = {}
    _, x, img, nd = _traj(SM, fn, "dpmpp2m", "edm", "dpm2m_edm", ae=ae)
    arrays.update(x_dpmpp2m_edm=x, img_dpmpp2m_edm=img)
    B, L = TRAJ["B"], TRAJ["L"]
    imgin = synth_input("sxi2i.img", (B, 3, 2 * L, 2 * L), SEED, 0.5).clamp(-1, 1)
    enc_noise = synth_input("sxi2i.enc_noise", (B, 4, L, L), SEED)
    fwd_noise = synth_input("sxi2i.noise", (B, 4, L, L), SEED)
    S, k = EXTRA["i2i_steps"], EXTRA["i2i_strength"]
    smp = make(SM, "dpmpp2s_ancestral", "edm", S, TRAJ["cfg"])
    smp.discretization = I2I(smp.discretization, strength=k)
    with fp32_forward():
        post = DiagonalGaussianDistribution(ae.quant_conv(ae.encoder(imgin)))
        z = 0.13025 * (post.mean + post.std * enc_noise)
        sigmas = smp.discretization(S)
        noised_z = (z + fwd_noise * sigmas[0]) / torch.sqrt(1.0 + sigmas[0] ** 2.0)
    _, x, img, nd = _traj(SM, fn, "dpmpp2s_ancestral", "edm", "sxi2i", steps=S, wrapper=("i2i", k), I2I=I2I, x_in=noised_z, ae=ae)
    arrays.update(z_i2i=z, sigmas_i2i=sigmas, x_i2i=x, img_i2i=img)
    meta["draws"]["i2i"] = nd
    S, k = EXTRA["t2n_steps"], EXTRA["t2n_strength"]
    smp, x, _, nd = _traj(SM, fn, "heun_edm", "edm", "sxt2n", steps=S, wrapper=("t2n", k), T2N=T2N, decode=False)
    arrays.update(x_t2n=x, sigmas_t2n=smp.discretization(S))
    meta["draws"]["t2n"] = nd
    save("traj_sdxl_samplers_extra", meta, **arrays)


CASES = {"sdxl_samplers_sched": g_sdxl_samplers_sched, "sdxl_samplers_toy": g_sdxl_samplers_toy,
         **{f"traj_sdxl_{k}": (lambda k=k: _g_traj(k)) for k in NEW}, "traj_sdxl_samplers_extra": g_traj_sdxl_samplers_extra}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", nargs="*")
    a = ap.parse_args()
    torch.manual_seed(0)
    for name, fn in CASES.items():
        if a.only and name not in a.only:
            continue
        fn()


if __name__ == "__main__":
    main()
