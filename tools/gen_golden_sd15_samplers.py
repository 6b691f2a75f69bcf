"""ORACLE tooling for the rest of Cremage's SD1.5 sampler menu (Heun, DPM2, DPM2 A, LMS, DPM++ 2S A, DPM++ SDE, DPM++ 2M, DPM++ 2M SDE,
DPM++ 3M SDE) - writes tests/golden/{sd15_samplers_sched, sd15_samplers_toy, traj_sd15_<key> (nine), traj_sd15_hires_dpmpp_2m}.npz from
the reference's own modules (k_diffusion.sampling's sample_* functions and get_sigmas_karras, Cremage's sampler classes of
ldm/models/diffusion/k_diffusion_samplers.py, LDMWrapperForKDiffusion, CompVisDenoiser, LatentDiffusion), on the name-keyed synthetic
weights and `synth_input` tensors of oracle/gen_golden.py, whose import stubs and helpers it reuses (that module is imported, not
changed).  Every noise draw is a recorded tensor `synth_input(f"{tag}.noise{k}")` handed out by a noise sampler that also records the
(sigma, sigma_next) it was called with.  Only the .npz files are committed; a rerun reproduces the arrays exactly.

    python tools/gen_golden_sd15_samplers.py [--only NAME ...]
"""
import argparse
import contextlib
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from oracle import gen_golden as G  # noqa: E402  (installs the import stubs and puts the reference on sys.path)
from oracle.gen_golden import R_ks, R_ksamp, SEED, fp32_forward, save, synth_input  # noqa: E402

from cremage.utils.sampler_utils import sampler_name_list  # noqa: E402  (the menu itself)

SIGMA_MIN, SIGMA_MAX = 0.0316386, 14.5521805  # KDiffusionSamplerBase's defaults (k_diffusion_samplers.py:66-67)
# key -> (k_diffusion function, Cremage's class, schedule)
SAMPLERS = {"heun": ("sample_heun", "HeunSampler", "model"), "dpm2": ("sample_dpm_2", "Dpm2Sampler", "karras"),
            "dpm2_a": ("sample_dpm_2_ancestral", "Dpm2AncestralSampler", "karras"), "lms": ("sample_lms", "LmsSampler", "model"),
            "dpmpp_2s_a": ("sample_dpmpp_2s_ancestral", "Dpmpp2sAncestralSampler", "karras"),
            "dpmpp_sde": ("sample_dpmpp_sde", "DpmppSdeSampler", "karras"), "dpmpp_2m": ("sample_dpmpp_2m", "Dpmpp2mSampler", "karras"),
            "dpmpp_2m_sde": ("sample_dpmpp_2m_sde", "Dpmpp2mSdeSampler", "karras"),
            "dpmpp_3m_sde": ("sample_dpmpp_3m_sde", "Dpmpp3mSdeSampler", "karras")}
TAKES_NOISE = ("dpm2_a", "dpmpp_2s_a", "dpmpp_sde", "dpmpp_2m_sde", "dpmpp_3m_sde")
SDE = ("dpmpp_sde", "dpmpp_2m_sde", "dpmpp_3m_sde")


class Recorded:
    """noise_sampler(sigma, sigma_next) -> synth_input(f"{tag}.noise{k}") for the k-th call; keeps the calls' arguments."""

    def __init__(self, tag, shape):
        self.tag, self.shape, self.calls, self.noise = tag, tuple(shape), [], []

    def __call__(self, sigma, sigma_next):
        z = synth_input(f"{self.tag}.noise{len(self.calls)}", self.shape, SEED)
        self.calls.append([float(sigma), float(sigma_next)])
        self.noise.append(z)
        return z

    def arrays(self):
        return (torch.tensor(self.calls, dtype=torch.float32).reshape(-1, 2),
                torch.stack(self.noise) if self.noise else torch.zeros((0,) + self.shape))


def _quiet():
    R_ks.trange = R_ksamp.trange = lambda *a, **k: range(*a)  # silence tqdm


SCHED_STEPS = [1, 2, 6, 20]


def g_sd15_samplers_sched():
    """get_sigmas_karras with Cremage's sigma_min / sigma_max, and the menu's names."""
    arrays = {f"karras_{n}": R_ksamp.get_sigmas_karras(n, SIGMA_MIN, SIGMA_MAX) for n in SCHED_STEPS}
    save("sd15_samplers_sched", dict(steps=SCHED_STEPS, sigma_min=SIGMA_MIN, sigma_max=SIGMA_MAX, rho=7.0, names=list(sampler_name_list)),
         **arrays)


TOY = dict(B=2, shape=[4, 9, 11], cfg=7.5, steps=[1, 2, 3, 7])


def toy_model(cu, cc, cfg):
    """Analytic stand-in for LDMWrapperForKDiffusion(CompVisDenoiser): two eps branches (a linear and a softsign one), eps-scaled as
    CompVisDenoiser does (den = x - sigma * eps), and guidance on the denoised values.  Both eps are bounded, so den -> x and the
    ODE derivative (x - den) / sigma stays O(1) as sigma -> 0, as with every eps model; a toy whose denoised value does not approach
    its input lets that derivative grow like 1 / sigma and multiplies a one-ulp difference of an LMS coefficient by hundreds.
    Only correctly rounded operations (+ - * / abs) are used: tanh or exp differ in the last bit from one CPU to the next.
    Restated in tests/test_sd15_samplers_cpu.py."""
    def model(x, sigma):
        s = sigma.reshape(-1, 1, 1, 1)
        eps_u = x * (s / (1.0 + s ** 2)) - cu.reshape(-1, 4, 1, 1) / (1.0 + s)
        u = x * (s / (1.0 + s ** 2))
        eps_c = u / (1.0 + u.abs()) - cc.reshape(-1, 4, 1, 1) / (1.0 + s)
        den_u, den_c = x - s * eps_u, x - s * eps_c
        return den_u + cfg * (den_c - den_u)
    return model


def g_sd15_samplers_toy():
    """Each sample_* function under toy_model with recorded noise: final latents, the schedule, and the noise calls' arguments.  A
    function that raises is listed in `raises` with the exception's name (the two multistep SDE samplers at one step)."""
    _quiet()
    B, shape, cfg = TOY["B"], tuple(TOY["shape"]), TOY["cfg"]
    cu, cc = synth_input("sd15toy.cu", (B, 4), SEED), synth_input("sd15toy.cc", (B, 4), SEED)
    x0 = synth_input("sd15toy.x0", (B,) + shape, SEED)
    model = toy_model(cu, cc, cfg)
    den = G.R_kext.CompVisDenoiser(G._tiny_ldm(), False)
    arrays, raises = {}, {}
    for key, (fn, _, sched) in SAMPLERS.items():
        for n in TOY["steps"]:
            sigmas = den.get_sigmas(n) if sched == "model" else R_ksamp.get_sigmas_karras(n, SIGMA_MIN, SIGMA_MAX)
            rec = Recorded(f"sd15toy.{key}.{n}", (B,) + shape)
            kw = dict(noise_sampler=rec) if key in TAKES_NOISE else {}
            torch.manual_seed(0)
            try:
                with torch.no_grad():
                    x = getattr(R_ksamp, fn)(model, x0.clone(), sigmas, **kw)
            except UnboundLocalError as e:
                raises[f"{key}_{n}"] = type(e).__name__
                continue
            arrays[f"x_{key}_{n}"], arrays[f"sig_{key}_{n}"], arrays[f"calls_{key}_{n}"] = x, sigmas, rec.arrays()[0]
    save("sd15_samplers_toy", dict(TOY, seed=SEED, keys=list(SAMPLERS), raises=raises), x0=x0, **arrays)


TRAJ = dict(B=2, L=16, S=6, cfg=7.5)


def _cremage_sampler(ldm, key):
    """Cremage's sampler object with fp32 schedule buffers (see oracle/gen_golden.py g_hires_latent for the shim)."""
    orig_rb = R_ks.KDiffusionSamplerBase.register_buffer
    R_ks.KDiffusionSamplerBase.register_buffer = lambda self, name, attr: setattr(self, name, attr)
    try:
        with fp32_forward():
            return getattr(R_ks, SAMPLERS[key][1])(ldm)
    finally:
        R_ks.KDiffusionSamplerBase.register_buffer = orig_rb


def _run(s, key, rec):
    """do_sample of Cremage's class with the recording noise sampler as k-diffusion's default one; the SDE trio through its sample_*
    function directly, since do_sample would build a torchsde Brownian tree."""
    if key in SDE:
        return getattr(R_ksamp, SAMPLERS[key][0])(s.ldm_wrapper_model, s.x, s.sigmas, noise_sampler=rec)
    orig = R_ksamp.default_noise_sampler
    R_ksamp.default_noise_sampler = lambda x: rec
    try:
        return s.do_sample()[0]
    finally:
        R_ksamp.default_noise_sampler = orig


def _g_traj(key):
    """TRAJ["S"] steps of `key` on the tiny LDM of traj_euler (CFG 7.5) and the first stage's decode."""
    _quiet()
    ldm = G._tiny_ldm()
    B, L, S, cfg = TRAJ["B"], TRAJ["L"], TRAJ["S"], TRAJ["cfg"]
    c, uc = synth_input("traj.c", (B, 77, 96), SEED), synth_input("traj.uc", (B, 77, 96), SEED)
    x0 = synth_input("traj.x0", (B, 4, L, L), SEED)
    rec = Recorded(f"sd15.{key}", (B, 4, L, L))
    s = _cremage_sampler(ldm, key)
    torch.manual_seed(0)
    with fp32_forward(), contextlib.redirect_stdout(open(os.devnull, "w")):
        s._sample_common_prep(S=S, batch_size=B, shape=[4, L, L], conditioning=c, unconditional_guidance_scale=cfg,
                              unconditional_conditioning=uc, x0=x0)
        x = _run(s, key, rec)
        img = ldm.decode_first_stage(x)
    calls, noise = rec.arrays()
    save(f"traj_sd15_{key}", dict(TRAJ, key=key, seed=SEED, unet=G.TINY_UNET, dd=G.TINY_DD, draws=len(rec.calls)),
         sigmas=s.sigmas, x=x, img=img, calls=calls, noise=noise)


def g_traj_sd15_hires_dpmpp_2m():
    """oracle/gen_golden.py g_hires_latent's flow with DPM++ 2M: the Karras schedule, stochastic_encode and `denoising_steps`."""
    _quiet()
    ldm = G._tiny_ldm()
    B, L, S, factor, strength = 2, 8, 6, 2, 0.5
    c, uc = synth_input("hires.c", (B, 77, 96), SEED), synth_input("hires.uc", (B, 77, 96), SEED)
    x0 = synth_input("hires.x0", (B, 4, L, L), SEED)
    noise = synth_input("hires.noise", (B, 4, factor * L, factor * L), SEED)
    t_enc = int(strength * S)
    s = _cremage_sampler(ldm, "dpmpp_2m")
    assert s.sqrt_alphas_cumprod.dtype == torch.float32
    with fp32_forward(), contextlib.redirect_stdout(open(os.devnull, "w")):
        s._sample_common_prep(S=S, batch_size=B, shape=[4, L, L], conditioning=c, unconditional_guidance_scale=7.5,
                              unconditional_conditioning=uc, x0=x0)
        base, _ = s.do_sample()
        up = torch.nn.functional.interpolate(base, scale_factor=factor, mode="bilinear", align_corners=False)
        z_enc = s.stochastic_encode(up, torch.tensor([t_enc] * B), sampling_steps=S, noise=noise)
        s._sample_common_prep(S=S, batch_size=B, shape=[4, factor * L, factor * L], conditioning=c, unconditional_guidance_scale=7.5,
                              unconditional_conditioning=uc, x0=z_enc, denoising_steps=t_enc)
        x, _ = s.do_sample()
        img = ldm.decode_first_stage(x)
    save("traj_sd15_hires_dpmpp_2m", dict(B=B, L=L, S=S, factor=factor, strength=strength, t_enc=t_enc, cfg=7.5, seed=SEED,
                                          unet=G.TINY_UNET, dd=G.TINY_DD),
         base=base, up=up, z_enc=z_enc, sigmas=s.sigmas, x=x, img=img)


CASES = {"sd15_samplers_sched": g_sd15_samplers_sched, "sd15_samplers_toy": g_sd15_samplers_toy,
         **{f"traj_sd15_{k}": (lambda k=k: _g_traj(k)) for k in SAMPLERS}, "traj_sd15_hires_dpmpp_2m": g_traj_sd15_hires_dpmpp_2m}


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
