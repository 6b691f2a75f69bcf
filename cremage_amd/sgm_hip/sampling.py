"""SDXL denoiser / guider / sampler glue - stays on PyTorch (north_star), behaviour of
modules/sdxl/sgm/modules/diffusionmodules/{denoiser.py:10-75, denoiser_scaling.py:29-37, discretizer.py:17-78,
guiders.py:24-65, sampling.py:29-573, sampling_utils.py:7-51, wrappers.py:24-34} and DiffusionEngine.decode_first_stage
(sgm/models/diffusion.py:118-136).  Tensors here are [b, 4, L, L] latents and per-sample scalars; the per-step cost
is the UNet call.  Every sampler but EulerEDM is a plan run by cremage_amd.sampler_plan's executors (what the SD1.5 k-diffusion
samplers run through as well); the scalar tables the plans are built from live there and are re-exported here."""
from __future__ import annotations

from typing import Dict, Optional

import numpy as np
import torch
import torch.nn as nn

from ..sampler_plan import (EDMDiscretization, ancestral_table, append_zero, doubled_input, dpmpp2m_multipliers, edm_table,  # noqa: F401
                            get_ancestral_step, linear_multistep_coeff, lms_table, plan_dpmpp_2m, plan_dpmpp_2s_a, plan_euler_a, plan_heun,
                            plan_lms, run_plan)
from ..samplers import append_dims, make_beta_schedule


class LegacyDDPMDiscretization:
    """discretizer.py:51-78 (+ Discretization.__call__ :17-24)."""

    def __init__(self, linear_start=0.00085, linear_end=0.0120, num_timesteps=1000):
        self.num_timesteps = num_timesteps
        betas = make_beta_schedule("linear", num_timesteps, linear_start=linear_start, linear_end=linear_end)
        self.alphas_cumprod = np.cumprod(1.0 - betas, axis=0)

    def get_sigmas(self, n, device="cpu"):
        if n < self.num_timesteps:
            timesteps = np.linspace(self.num_timesteps - 1, 0, n, endpoint=False).astype(int)[::-1]
            alphas_cumprod = self.alphas_cumprod[timesteps]
        elif n == self.num_timesteps:
            alphas_cumprod = self.alphas_cumprod
        else:
            raise ValueError
        sigmas = torch.tensor((1 - alphas_cumprod) / alphas_cumprod, dtype=torch.float32, device=device) ** 0.5
        return torch.flip(sigmas, (0,))

    def __call__(self, n, do_append_zero=True, device="cpu", flip=False):
        sigmas = self.get_sigmas(n, device=device)
        sigmas = append_zero(sigmas) if do_append_zero else sigmas
        return sigmas if not flip else torch.flip(sigmas, (0,))


# Cremage's sampler preferences (cremage/configs/preferences.py:149-165) and what they default to
SAMPLER_OPTION_DEFAULTS = {"sampler_s_churn": 0.0, "sampler_s_tmin": 0.0, "sampler_s_tmax": 999.0, "sampler_s_noise": 1.0,
                           "sampler_eta": 1.0, "sampler_order": 4, "discretization_sigma_min": 0.0292, "discretization_sigma_max": 14.6146,
                           "discretization_rho": 3.0}
DISCRETIZATIONS = {"legacy_ddpm": "legacy_ddpm", "LegacyDDPMDiscretization": "legacy_ddpm", "edm": "edm", "EDMDiscretization": "edm"}


def sampler_options(options: Optional[Dict] = None) -> Dict:
    """SAMPLER_OPTION_DEFAULTS overridden by `options` (keyed by the preference names); an unknown name is an error."""
    unknown = set(options or {}) - set(SAMPLER_OPTION_DEFAULTS)
    if unknown:
        raise ValueError(f"unknown sampler options {sorted(unknown)} (known: {sorted(SAMPLER_OPTION_DEFAULTS)})")
    return dict(SAMPLER_OPTION_DEFAULTS, **(options or {}))


def make_discretization(name: str = "legacy_ddpm", options: Optional[Dict] = None):
    """get_discretization_config (sdxl_image_generator_utils.py:418-449): "legacy_ddpm" / "edm" (or Cremage's class names)."""
    if name not in DISCRETIZATIONS:
        raise ValueError(f"unknown discretization {name!r} (one of {sorted(DISCRETIZATIONS)})")
    if DISCRETIZATIONS[name] == "legacy_ddpm":
        return LegacyDDPMDiscretization()
    o = sampler_options(options)
    return EDMDiscretization(sigma_min=o["discretization_sigma_min"], sigma_max=o["discretization_sigma_max"], rho=o["discretization_rho"])


class EpsScaling:
    """denoiser_scaling.py:29-37."""

    def __call__(self, sigma):
        c_skip = torch.ones_like(sigma, device=sigma.device)
        c_out = -sigma
        c_in = 1 / (sigma ** 2 + 1.0) ** 0.5
        c_noise = sigma.clone()
        return c_skip, c_out, c_in, c_noise


class DiscreteDenoiser(nn.Module):
    """denoiser.py:10-75: sigma (and c_noise) quantised to the 1000-entry DDPM table; c_noise becomes the table index."""

    def __init__(self, num_idx: int = 1000, quantize_c_noise: bool = True):
        super().__init__()
        self.scaling = EpsScaling()
        self.discretization = LegacyDDPMDiscretization()
        self.register_buffer("sigmas", self.discretization(num_idx, do_append_zero=False, flip=True))
        self.quantize_c_noise = quantize_c_noise
        self.num_idx = num_idx

    def sigma_to_idx(self, sigma):
        dists = sigma - self.sigmas[:, None]
        return dists.abs().argmin(dim=0).view(sigma.shape)

    def idx_to_sigma(self, idx):
        return self.sigmas[idx]

    def forward(self, network, input, sigma, cond: Dict, **additional_model_inputs):
        sigma = self.idx_to_sigma(self.sigma_to_idx(sigma))
        sigma_shape = sigma.shape
        sigma = append_dims(sigma, input.ndim)
        c_skip, c_out, c_in, c_noise = self.scaling(sigma)
        c_noise = c_noise.reshape(sigma_shape)
        if self.quantize_c_noise:
            c_noise = self.sigma_to_idx(c_noise)
        return network(input * c_in, c_noise, cond, **additional_model_inputs) * c_out + input * c_skip


class VanillaCFG:
    """guiders.py:24-65.  The concatenated conditioning is built once per (c, uc) pair and reused every step
    (the reference re-concatenates identical tensors each step), which keeps the cross-attention K/V cache hot."""

    def __init__(self, scale: float):
        self.scale = scale
        self._cache = None

    def __call__(self, x, sigma):
        x_u, x_c = x.chunk(2)
        return x_u + self.scale * (x_c - x_u)

    def cat_cond(self, c, uc):
        """The batch-doubled conditioning dict of prepare_inputs, built once per (c, uc) pair."""
        k = self._cache
        if k is None or k[0] is not c or k[1] is not uc:
            c_out = dict()
            for key in c:
                if key in ["vector", "crossattn", "concat"]:
                    c_out[key] = torch.cat((uc[key], c[key]), 0)
                else:
                    assert c[key] == uc[key]
                    c_out[key] = c[key]
            self._cache = k = (c, uc, c_out)
        return k[2]

    def prepare_inputs(self, x, s, c, uc):
        return torch.cat([x] * 2), torch.cat([s] * 2), self.cat_cond(c, uc)


class OpenAIWrapper(nn.Module):
    """wrappers.py:24-34."""

    def __init__(self, diffusion_model):
        super().__init__()
        self.diffusion_model = diffusion_model

    def forward(self, x, t, c: dict, **kwargs):
        if "concat" in c:
            x = torch.cat((x, c["concat"]), dim=1)
        return self.diffusion_model(x, timesteps=t, context=c.get("crossattn", None), y=c.get("vector", None), **kwargs)


class Img2ImgDiscretizationWrapper:
    """scripts/demo/discretization.py:11-32 (installed on the sampler by init_sampling, sdxl_image_generator_utils.py:398-403):
    keeps the last max(int(strength * len), 1) sigmas of the descending list, i.e. img2img starts part-way down the schedule."""

    def __init__(self, discretization, strength: float = 1.0):
        assert 0.0 <= strength <= 1.0
        self.discretization = discretization
        self.strength = strength

    def __call__(self, *args, **kwargs):
        sigmas = torch.flip(self.discretization(*args, **kwargs), (0,))
        sigmas = sigmas[: max(int(self.strength * len(sigmas)), 1)]
        return torch.flip(sigmas, (0,))


class Txt2NoisyDiscretizationWrapper:
    """scripts/demo/discretization.py:35-95 (installed by init_sampling for a base stage that a refiner finishes,
    sdxl_image_generator_utils.py:404-407): drops the last max(min(int(strength * steps) - 1, steps - 1), 0) sigmas of the schedule,
    steps = original_steps + 1 when given, else the schedule's length; strength 0 keeps the whole schedule."""

    def __init__(self, discretization, strength: float = 0.0, original_steps=None):
        assert 0.0 <= strength <= 1.0
        self.discretization = discretization
        self.strength = strength
        self.original_steps = original_steps

    def __call__(self, *args, **kwargs):
        sigmas = torch.flip(self.discretization(*args, **kwargs), (0,))
        steps = len(sigmas) if self.original_steps is None else self.original_steps + 1
        prune_index = max(min(int(self.strength * steps) - 1, steps - 1), 0)
        return torch.flip(sigmas[prune_index:], (0,))


def wrap_discretization(discretization, steps: int, img2img_strength: Optional[float] = None, stage2strength: Optional[float] = None):
    """init_sampling's wrapping order (sdxl_image_generator_utils.py:398-407): Img2Img first, then Txt2Noisy around it."""
    if img2img_strength is not None:
        discretization = Img2ImgDiscretizationWrapper(discretization, strength=img2img_strength)
    if stage2strength is not None:
        discretization = Txt2NoisyDiscretizationWrapper(discretization, strength=stage2strength, original_steps=steps)
    return discretization


class EulerEDMSampler:
    """sampling.py:29-219,309-318 with s_churn = 0 (the reference's default): Euler steps on the EDM ODE."""

    def __init__(self, num_steps: int, guider: VanillaCFG, device="cuda", s_churn=0.0, s_tmin=0.0, s_tmax=float("inf"), s_noise=1.0):
        self.num_steps = num_steps
        self.discretization = LegacyDDPMDiscretization()
        self.guider = guider
        self.device = device
        self.s_churn, self.s_tmin, self.s_tmax, self.s_noise = s_churn, s_tmin, s_tmax, s_noise

    def denoise(self, x, denoiser, sigma, cond, uc):
        denoised = denoiser(*self.guider.prepare_inputs(x, sigma, cond, uc))
        return self.guider(denoised, sigma)

    @torch.no_grad()
    def __call__(self, denoiser, x, cond, uc=None, num_steps=None):
        n = self.num_steps if num_steps is None else num_steps
        sigmas = self.discretization(n, device=self.device)
        # CPU twin of the schedule for everything that steers the loop: a 0-dim device tensor in a Python comparison is a
        # stream synchronisation per step (cremage_amd.samplers._host_sigmas)
        sh = self.discretization(n, device="cpu").float()
        uc = cond if uc is None else uc
        x = x * float(torch.sqrt(1.0 + sh[0] ** 2.0))
        num_sigmas = len(sigmas)
        s_in = x.new_ones([x.shape[0]])
        for i in range(num_sigmas - 1):
            gamma = min(self.s_churn / (num_sigmas - 1), 2 ** 0.5 - 1) if self.s_tmin <= sh[i].item() <= self.s_tmax else 0.0
            sigma_hat_h = sh[i] * (gamma + 1.0)
            sigma_hat = s_in * (sigmas[i] * (gamma + 1.0))
            if gamma > 0:
                eps = torch.randn_like(x) * self.s_noise
                x = x + eps * float((sigma_hat_h ** 2 - sh[i] ** 2) ** 0.5)
            denoised = self.denoise(x, denoiser, sigma_hat, cond, uc)
            d = (x - denoised) / sigma_hat_h.item()
            x = x + (sh[i + 1] - sigma_hat_h).item() * d
        return x


def snap_to_table(table: torch.Tensor, sigmas: torch.Tensor) -> torch.Tensor:
    """DiscreteDenoiser.sigma_to_idx (denoiser.py:54-56) of every sigma at once, on the CPU: the index of the nearest table entry."""
    return (sigmas - table[:, None]).abs().argmin(dim=0)


class _DiscreteEvals:
    """The fused plan executor's evaluator (sampler_plan) over the engine's DiscreteDenoiser `dd` and network, with the guider's doubled
    conditioning `cc` and scale `cfg`.  fused_evals, once per run: DiscreteDenoiser.sigma_to_idx for all evaluation sigmas at once, the
    snapped sigmas (c_out = -sq), c_in with the per-call path's device arithmetic and the timestep rows (the table indices; the SDXL
    UNet hoists no timestep work).  Per evaluation one input build and the network."""

    def __init__(self, dd: "DiscreteDenoiser", network, cc: Dict, cfg: float):
        self.table, self.network, self.cc, self.cfg = dd.sigmas.detach().cpu(), network, cc, cfg

    def fused_evals(self, ev: torch.Tensor, x: torch.Tensor):
        idx = snap_to_table(self.table, ev)
        sq = self.table[idx]
        self.c_out = [-v for v in sq.tolist()]
        self.c_in = 1 / (sq.to(x.device) ** 2 + 1.0) ** 0.5
        self.t_rows = idx.to(x.device).reshape(-1, 1).expand(-1, 2 * x.shape[0]).contiguous()
        return self

    def __call__(self, k: int, xin: torch.Tensor):
        return self.network(doubled_input(xin, self.c_in[k]), self.t_rows[k], self.cc).contiguous(), self.c_out[k]


class _KSampler:
    """The five samplers that run as plans (cremage_amd.sampler_plan): the schedule on the CPU (what steers the run),
    prepare_sampling_loop's `x *= sqrt(1 + sigma_0^2)` on a copy (the caller's tensor is not mutated), the sampler's plan over that
    schedule, and the choice of executor.  Fused (CUDA fp32 latents, VanillaCFG with scale != 1, the engine's denoiser and network as
    `parts`): per UNet evaluation one input build, the network and one fused step launch, which does the denoiser scalings, the guidance
    and the update.  Otherwise the torch executor around `denoise`, which restates the reference and runs on the CPU as well."""

    def __init__(self, num_steps: int, guider: VanillaCFG, device="cuda", fused: bool = True):
        self.num_steps = num_steps
        self.discretization = LegacyDDPMDiscretization()
        self.guider = guider
        self.device = device
        self.fused = fused

    def denoise(self, x, denoiser, sigma, cond, uc):
        denoised = denoiser(*self.guider.prepare_inputs(x, sigma, cond, uc))
        return self.guider(denoised, sigma)

    def fused_ok(self, x, parts) -> bool:
        return (self.fused and parts is not None and x.is_cuda and x.dtype == torch.float32 and isinstance(self.guider, VanillaCFG)
                and self.guider.scale != 1.0)

    def plan(self, sh, b):
        """The run's plan over the CPU fp32 schedule `sh` for a batch of b."""
        raise NotImplementedError

    @torch.no_grad()
    def __call__(self, denoiser, x, cond, uc=None, num_steps=None, parts=None):
        """`parts` = (DiscreteDenoiser, network): the pieces `denoiser` applies, for the fused path."""
        n = self.num_steps if num_steps is None else num_steps
        sh = self.discretization(n, device="cpu").float()
        uc = cond if uc is None else uc
        x = x * float(torch.sqrt(1.0 + sh[0] ** 2.0))
        fused = self.fused_ok(x, parts)
        if fused:
            model = _DiscreteEvals(parts[0], parts[1], self.guider.cat_cond(cond, uc), self.guider.scale)
        else:
            model = lambda xin, sigma: self.denoise(xin, denoiser, sigma, cond, uc)  # noqa: E731
        return run_plan(model, x, self.plan(sh, x.shape[0]), fused=fused)


class DPMPP2MSampler(_KSampler):
    """sampling.py:29-137,459-573: DPM++ 2M (multistep, second order) with CFG, Cremage's default SDXL sampler (preferences.py:159);
    fused step: crg_cfg_dpmpp2m_step."""

    def plan(self, sh, b):
        return plan_dpmpp_2m(sh)


class HeunEDMSampler(_KSampler):
    """sampling.py:147-219,321-358: Heun steps on the EDM ODE, two UNet calls per step (one when the next sigma is 0), with the EDM
    churn (s_churn > 0: noise drawn and added before the first call of the steps where gamma > 0)."""

    def __init__(self, num_steps: int, guider: VanillaCFG, device="cuda", s_churn=0.0, s_tmin=0.0, s_tmax=float("inf"), s_noise=1.0,
                 fused: bool = True):
        super().__init__(num_steps, guider, device, fused)
        self.s_churn, self.s_tmin, self.s_tmax, self.s_noise = s_churn, s_tmin, s_tmax, s_noise

    def plan(self, sh, b):
        return plan_heun(sh, s_noise=self.s_noise, b=b, s_churn=self.s_churn, s_tmin=self.s_tmin, s_tmax=self.s_tmax, sgm=True)


class _AncestralSampler(_KSampler):
    """sampling.py:222-268: eta, s_noise, and one torch.randn_like(x) per step - the last step's included, which the reference's
    torch.where throws away."""

    def __init__(self, num_steps: int, guider: VanillaCFG, device="cuda", eta=1.0, s_noise=1.0, fused: bool = True):
        super().__init__(num_steps, guider, device, fused)
        self.eta, self.s_noise = eta, s_noise


class EulerAncestralSampler(_AncestralSampler):
    """sampling.py:361-381: an Euler step to sigma_down, then noise of std sigma_up."""

    def plan(self, sh, b):
        return plan_euler_a(sh, self.eta, self.s_noise, b=b, sgm=True)


class DPMPP2SAncestralSampler(_AncestralSampler):
    """sampling.py:384-456: DPM++ 2S ancestral - a second UNet call at the midpoint sigma to_sigma(s) (off the denoiser's grid: it is
    snapped for the scalings only), then noise of std sigma_up; a step whose sigma_down is 0 makes one call (the Euler step)."""

    def plan(self, sh, b):
        return plan_dpmpp_2s_a(sh, self.eta, self.s_noise, b=b, sgm=True)


class LinearMultistepSampler(_KSampler):
    """sampling.py:271-306: linear multistep of the given order over the last derivatives (coefficients: lms_table).  The fused step
    reads at most three earlier derivatives, so it covers order <= 4; a larger order runs the torch executor."""

    FUSED_MAX_ORDER = 4

    def __init__(self, num_steps: int, guider: VanillaCFG, device="cuda", order=4, fused: bool = True):
        super().__init__(num_steps, guider, device, fused)
        if int(order) < 1:
            raise ValueError(f"LMS order must be >= 1 (got {order})")
        self.order = int(order)

    def fused_ok(self, x, parts) -> bool:
        return self.order <= self.FUSED_MAX_ORDER and super().fused_ok(x, parts)

    def plan(self, sh, b):
        return plan_lms(sh, order=self.order)


SGM_SAMPLERS = {"euler_edm": EulerEDMSampler, "dpmpp2m": DPMPP2MSampler, "heun_edm": HeunEDMSampler,
                "euler_ancestral": EulerAncestralSampler, "dpmpp2s_ancestral": DPMPP2SAncestralSampler,
                "linear_multistep": LinearMultistepSampler}  # get_sampler, sdxl_image_generator_utils.py:451-522
# Cremage's SDXL sampler menu (modules/sdxl/const/const.py:37-45; init_sampling appends "Sampler") -> SGM_SAMPLERS keys
CREMAGE_SAMPLER_KEYS = {"EulerEDM": "euler_edm", "HeunEDM": "heun_edm", "EulerAncestral": "euler_ancestral",
                        "DPMPP2SAncestral": "dpmpp2s_ancestral", "DPMPP2M": "dpmpp2m", "LinearMultistep": "linear_multistep"}
CREMAGE_SAMPLER_KEYS.update({k + "Sampler": v for k, v in list(CREMAGE_SAMPLER_KEYS.items())})
# the options each sampler takes (get_sampler): constructor argument <- preference name
_SAMPLER_OPTION_ARGS = {"euler_edm": dict(s_churn="sampler_s_churn", s_tmin="sampler_s_tmin", s_tmax="sampler_s_tmax", s_noise="sampler_s_noise"),
                        "heun_edm": dict(s_churn="sampler_s_churn", s_tmin="sampler_s_tmin", s_tmax="sampler_s_tmax", s_noise="sampler_s_noise"),
                        "euler_ancestral": dict(eta="sampler_eta", s_noise="sampler_s_noise"),
                        "dpmpp2s_ancestral": dict(eta="sampler_eta", s_noise="sampler_s_noise"),
                        "dpmpp2m": {}, "linear_multistep": dict(order="sampler_order")}


def sampler_key(name: str) -> str:
    """An SGM_SAMPLERS key, or Cremage's name for it ("HeunEDM", "HeunEDMSampler", ...), -> the key."""
    key = CREMAGE_SAMPLER_KEYS.get(name, name)
    if key not in SGM_SAMPLERS:
        raise ValueError(f"unknown SDXL sampler {name!r} (one of {sorted(SGM_SAMPLERS)} or {sorted(CREMAGE_SAMPLER_KEYS)})")
    return key


class DiffusionEngine(nn.Module):
    """Minimal stand-in for sgm/models/diffusion.py:19-151: model wrapper + denoiser + first stage + scale factor."""

    def __init__(self, unet: nn.Module, first_stage_model: nn.Module, scale_factor: float = 0.13025):
        super().__init__()
        self.model = OpenAIWrapper(unet)
        self.denoiser = DiscreteDenoiser()
        self.first_stage_model = first_stage_model
        self.scale_factor = scale_factor

    @torch.no_grad()
    def decode_first_stage(self, z):
        return self.first_stage_model.decode(1.0 / self.scale_factor * z)

    @torch.no_grad()
    def encode_first_stage(self, x, noise=None):
        """sgm/models/diffusion.py:139-151: scale_factor * posterior.sample() (the SDXL first stage is
        AutoencoderKLInferenceWrapper, whose encode samples the posterior); `noise` makes the sample explicit."""
        return self.scale_factor * self.first_stage_model.encode(x).sample(noise)

    def make_sampler(self, sampler: str, steps: int, cfg_scale: float, device, img2img_strength: Optional[float] = None,
                     stage2strength: Optional[float] = None, discretization: str = "legacy_ddpm", options: Optional[Dict] = None):
        """init_sampling (sdxl_image_generator_utils.py:359-415) for VanillaCFG: `sampler` an SGM_SAMPLERS key or Cremage's name
        (CREMAGE_SAMPLER_KEYS), `discretization` "legacy_ddpm" or "edm", `options` Cremage's sampler / discretization preferences
        (SAMPLER_OPTION_DEFAULTS; each sampler takes the ones get_sampler hands it)."""
        key = sampler_key(sampler)
        opts = sampler_options(options)
        kwargs = {arg: opts[pref] for arg, pref in _SAMPLER_OPTION_ARGS[key].items()}
        smp = SGM_SAMPLERS[key](steps, VanillaCFG(cfg_scale), device=device, **kwargs)
        smp.discretization = wrap_discretization(make_discretization(discretization, opts), steps, img2img_strength, stage2strength)
        return smp

    def run_sampler(self, smp, x, cond: Dict, uc: Dict):
        """sampler(denoiser, x, cond=c, uc=uc) (sdxl_image_generator_utils.py:703-707, :1016)."""
        denoiser = lambda inp, sigma, c: self.denoiser(self.model, inp, sigma, c)  # noqa: E731
        if isinstance(smp, _KSampler):
            return smp(denoiser, x, cond=cond, uc=uc, parts=(self.denoiser, self.model))
        return smp(denoiser, x, cond=cond, uc=uc)

    @torch.no_grad()
    def img2img(self, img, cond: Dict, uc: Dict, steps: int, strength: float, cfg_scale: float, enc_noise=None, fwd_noise=None,
                sampler: str = "euler_edm", stage2strength: Optional[float] = None, discretization: str = "legacy_ddpm",
                options: Optional[Dict] = None):
        """do_img2img, sdxl_image_generator_utils.py:989-1016 (the face-fix re-entry of BASELINE config 5 is this call on a crop,
        strength 0.3): encode, noise to sigma_0 of the pruned schedule, sample over the remaining sigmas.  `stage2strength`: the
        base stage of a refined run (Txt2Noisy around the Img2Img pruning); `discretization` / `options` as in make_sampler."""
        z = self.encode_first_stage(img, enc_noise)
        smp = self.make_sampler(sampler, steps, cfg_scale, z.device, img2img_strength=strength, stage2strength=stage2strength,
                                discretization=discretization, options=options)
        sigmas = smp.discretization(steps, device=z.device)
        noise = torch.randn_like(z) if fwd_noise is None else fwd_noise
        noised_z = (z + noise * sigmas[0]) / torch.sqrt(1.0 + sigmas[0] ** 2.0)
        return self.run_sampler(smp, noised_z, cond, uc)

    @torch.no_grad()
    def img2img_latent(self, z, cond: Dict, uc: Dict, steps: int, strength: float, cfg_scale: float, fwd_noise=None, factor: float = 1.0,
                       sampler: str = "euler_edm", discretization: str = "legacy_ddpm", options: Optional[Dict] = None):
        """do_img2img with skip_encode and add_noise (sdxl_image_generator_utils.py:986-1017) on latents z upscaled by `factor`
        (bilinear, align_corners False: the latent upscaler of the SDXL hires-fix, sdxl_image_generator.py:196-199): noise to
        sigma_0 of the Img2Img-pruned schedule, divide by sqrt(1 + sigma_0^2), sample over the remaining sigmas.  On fp32 device
        latents the upscale and the noising are ONE launch (ops.upscale_noise with host scalars); otherwise the torch expression
        of `img2img`.  `fwd_noise`: the noise, of the upscaled shape (randn by default)."""
        smp = self.make_sampler(sampler, steps, cfg_scale, z.device, img2img_strength=strength, discretization=discretization,
                                options=options)
        if z.is_cuda and z.dtype == torch.float32:
            from .. import ops
            s0 = smp.discretization(steps)[0]  # CPU fp32, the arithmetic of the device expression below
            if fwd_noise is None:
                fwd_noise = torch.randn((z.shape[0], z.shape[1], ops.upscaled_size(z.shape[2], factor),
                                         ops.upscaled_size(z.shape[3], factor)), device=z.device)
            noised_z = ops.upscale_noise(z.contiguous(), factor, fwd_noise.contiguous(), 1.0, float(s0),
                                         float(torch.sqrt(1.0 + s0 ** 2.0)))
        else:
            if factor != 1.0:
                z = torch.nn.functional.interpolate(z, scale_factor=factor, mode="bilinear", align_corners=False)
            sigmas = smp.discretization(steps, device=z.device)
            noise = torch.randn_like(z) if fwd_noise is None else fwd_noise
            noised_z = (z + noise * sigmas[0]) / torch.sqrt(1.0 + sigmas[0] ** 2.0)
        return self.run_sampler(smp, noised_z, cond, uc)

    @torch.no_grad()
    def sample(self, x, cond: Dict, uc: Dict, steps: int, cfg_scale: float, sampler: str = "euler_edm",
               stage2strength: Optional[float] = None, discretization: str = "legacy_ddpm", options: Optional[Dict] = None):
        """do_sample, sdxl_image_generator_utils.py:695-707: sampler(denoiser, randn, cond=c, uc=uc).  `stage2strength`: the base
        stage of a refined run, which stops early (Txt2NoisyDiscretizationWrapper); `discretization` / `options` as in make_sampler."""
        smp = self.make_sampler(sampler, steps, cfg_scale, x.device, stage2strength=stage2strength, discretization=discretization,
                                options=options)
        return self.run_sampler(smp, x, cond, uc)

    @torch.no_grad()
    def refine(self, z, cond: Dict, uc: Dict, steps: int, strength: float, cfg_scale: float, sampler: str = "dpmpp2m",
               discretization: str = "legacy_ddpm", options: Optional[Dict] = None):
        """The refiner stage: apply_refiner (sdxl_image_generator.py:307-347) -> do_img2img with skip_encode and no added noise
        (sdxl_image_generator_utils.py:986-1016, finish_denoising is always True, sdxl_image_generator.py:566): the base latents
        divided by sqrt(1 + sigma_0^2) of the Img2Img-pruned schedule, then the sampler over that schedule."""
        smp = self.make_sampler(sampler, steps, cfg_scale, z.device, img2img_strength=strength, discretization=discretization,
                                options=options)
        sigmas = smp.discretization(smp.num_steps).to(z.device)
        noised_z = z / torch.sqrt(1.0 + sigmas[0] ** 2.0)
        return self.run_sampler(smp, noised_z, cond, uc)
