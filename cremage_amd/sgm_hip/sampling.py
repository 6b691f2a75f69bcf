"""SDXL denoiser / guider / sampler glue - stays on PyTorch (north_star), behaviour of
modules/sdxl/sgm/modules/diffusionmodules/{denoiser.py:10-75, denoiser_scaling.py:29-37, discretizer.py:17-78,
guiders.py:24-65, sampling.py:29-219,309-318, wrappers.py:24-34} and DiffusionEngine.decode_first_stage
(sgm/models/diffusion.py:118-136).  Tensors here are [b, 4, L, L] latents and per-sample scalars; the per-step cost
is the UNet call."""
from __future__ import annotations

from typing import Dict, Optional

import numpy as np
import torch
import torch.nn as nn

from ..samplers import append_dims, append_zero, make_beta_schedule


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


def _to_neg_log_sigma(sigma):
    return sigma.log().neg()  # sampling_utils.py:46-47


def _to_sigma(neg_log_sigma):
    return neg_log_sigma.neg().exp()  # sampling_utils.py:50-51


def dpmpp2m_multipliers(sigmas: torch.Tensor):
    """Per step i of a DPM++ 2M run over the CPU fp32 schedule `sigmas`: (m1, m2, m3, m4, advanced) as Python floats holding fp32
    values.  The arithmetic is DPMPP2MSampler.get_variables / get_mult (sampling.py:460-486) op for op in fp32 torch on the CPU, so
    the scalars equal those of a CPU run of the reference bit for bit.  m3 / m4 are None on the first step; `advanced` is False on the
    first step and on a step whose next sigma is 0 (sampling.py:539-548)."""
    sigmas = sigmas.detach().to("cpu", torch.float32)
    out = []
    for i in range(len(sigmas) - 1):
        sigma, next_sigma = sigmas[i:i + 1], sigmas[i + 1:i + 2]
        t, t_next = _to_neg_log_sigma(sigma), _to_neg_log_sigma(next_sigma)
        h = t_next - t
        m1 = _to_sigma(t_next) / _to_sigma(t)
        m2 = (-h).expm1()
        m3 = m4 = None
        if i > 0:
            r = (t - _to_neg_log_sigma(sigmas[i - 1:i])) / h
            m3, m4 = float(1 + 1 / (2 * r)), float(1 / (2 * r))
        out.append((float(m1), float(m2), m3, m4, i > 0 and float(next_sigma) > 0.0))
    return out


class DPMPP2MSampler:
    """sampling.py:29-137,459-573: DPM++ 2M (multistep, second order) with CFG, Cremage's default SDXL sampler
    (preferences.py:159).  The schedule is computed once on the CPU (and moved to the device), the multipliers once per run
    (dpmpp2m_multipliers).  `x *= sqrt(1 + sigma_0^2)` is kept, on a copy: the caller's tensor is not mutated.

    Fused path (CUDA fp32 latents, VanillaCFG with scale != 1, the engine's denoiser and network passed as `parts`): per step one
    launch builds cat([x] * 2) * c_in, the network runs, and crg_cfg_dpmpp2m_step does the denoiser scalings, the guidance and the
    update in one launch.  Otherwise the torch loop below, which runs on the CPU as well."""

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

    @torch.no_grad()
    def __call__(self, denoiser, x, cond, uc=None, num_steps=None, parts=None):
        """`parts` = (DiscreteDenoiser, network): the pieces `denoiser` applies, for the fused path."""
        n = self.num_steps if num_steps is None else num_steps
        sh = self.discretization(n, device="cpu").float()
        uc = cond if uc is None else uc
        mults = dpmpp2m_multipliers(sh)
        x = x * float(torch.sqrt(1.0 + sh[0] ** 2.0))
        if self.fused_ok(x, parts):
            return self._fused(parts[0], parts[1], x.contiguous(), cond, uc, sh, mults)
        sigmas = sh.to(x.device)
        s_in = x.new_ones([x.shape[0]])
        old_denoised = None
        for i, (m1, m2, m3, m4, advanced) in enumerate(mults):
            denoised = self.denoise(x, denoiser, s_in * sigmas[i], cond, uc)
            if advanced:
                x = m1 * x - m2 * (m3 * denoised - m4 * old_denoised)
            else:
                x = m1 * x - m2 * denoised
            old_denoised = denoised
        return x

    def _fused(self, dd: "DiscreteDenoiser", network, x, cond, uc, sh, mults):
        from .. import ops
        b = x.shape[0]
        table = dd.sigmas.detach().cpu()
        idx = (sh[:-1] - table[:, None]).abs().argmin(dim=0)  # DiscreteDenoiser.sigma_to_idx for every step at once
        sq = table[idx]                                       # quantised sigmas: c_out = -sq
        c_in = 1 / (sq.to(x.device) ** 2 + 1.0) ** 0.5        # EpsScaling, the same device arithmetic as the per-step path
        t_rows = idx.to(x.device).reshape(-1, 1).expand(-1, 2 * b).contiguous()  # c_noise = sigma_to_idx(sigma_q)
        cc = self.guider.cat_cond(cond, uc)
        old = torch.empty_like(x)  # read from the second step on only
        for i, (m1, m2, m3, m4, advanced) in enumerate(mults):
            xx = torch.empty((2,) + tuple(x.shape), dtype=x.dtype, device=x.device)
            torch.mul(x.unsqueeze(0).expand_as(xx), c_in[i], out=xx)
            eps2 = network(xx.view((2 * b,) + tuple(x.shape[1:])), t_rows[i], cc)
            ops.cfg_dpmpp2m_step_(x, eps2.contiguous(), old, -float(sq[i]), self.guider.scale, m1, m2,
                                  0.0 if m3 is None else m3, 0.0 if m4 is None else m4, advanced)
        return x


SGM_SAMPLERS = {"euler_edm": EulerEDMSampler, "dpmpp2m": DPMPP2MSampler}  # sdxl_image_generator_utils.py:451-511 "EulerEDMSampler", "DPMPP2MSampler"


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
                     stage2strength: Optional[float] = None):
        """init_sampling (sdxl_image_generator_utils.py:359-415) for the LegacyDDPM discretization and VanillaCFG."""
        if sampler not in SGM_SAMPLERS:
            raise ValueError(f"unknown SDXL sampler {sampler!r} (one of {sorted(SGM_SAMPLERS)})")
        smp = SGM_SAMPLERS[sampler](steps, VanillaCFG(cfg_scale), device=device)
        smp.discretization = wrap_discretization(smp.discretization, steps, img2img_strength, stage2strength)
        return smp

    def run_sampler(self, smp, x, cond: Dict, uc: Dict):
        """sampler(denoiser, x, cond=c, uc=uc) (sdxl_image_generator_utils.py:703-707, :1016)."""
        denoiser = lambda inp, sigma, c: self.denoiser(self.model, inp, sigma, c)  # noqa: E731
        if isinstance(smp, DPMPP2MSampler):
            return smp(denoiser, x, cond=cond, uc=uc, parts=(self.denoiser, self.model))
        return smp(denoiser, x, cond=cond, uc=uc)

    @torch.no_grad()
    def img2img(self, img, cond: Dict, uc: Dict, steps: int, strength: float, cfg_scale: float, enc_noise=None, fwd_noise=None,
                sampler: str = "euler_edm", stage2strength: Optional[float] = None):
        """do_img2img, sdxl_image_generator_utils.py:989-1016 (the face-fix re-entry of BASELINE config 5 is this call on a crop,
        strength 0.3): encode, noise to sigma_0 of the pruned schedule, sample over the remaining sigmas.  `stage2strength`: the
        base stage of a refined run (Txt2Noisy around the Img2Img pruning)."""
        z = self.encode_first_stage(img, enc_noise)
        smp = self.make_sampler(sampler, steps, cfg_scale, z.device, img2img_strength=strength, stage2strength=stage2strength)
        sigmas = smp.discretization(steps, device=z.device)
        noise = torch.randn_like(z) if fwd_noise is None else fwd_noise
        noised_z = (z + noise * sigmas[0]) / torch.sqrt(1.0 + sigmas[0] ** 2.0)
        return self.run_sampler(smp, noised_z, cond, uc)

    @torch.no_grad()
    def sample(self, x, cond: Dict, uc: Dict, steps: int, cfg_scale: float, sampler: str = "euler_edm",
               stage2strength: Optional[float] = None):
        """do_sample, sdxl_image_generator_utils.py:695-707: sampler(denoiser, randn, cond=c, uc=uc).  `stage2strength`: the base
        stage of a refined run, which stops early (Txt2NoisyDiscretizationWrapper)."""
        smp = self.make_sampler(sampler, steps, cfg_scale, x.device, stage2strength=stage2strength)
        return self.run_sampler(smp, x, cond, uc)

    @torch.no_grad()
    def refine(self, z, cond: Dict, uc: Dict, steps: int, strength: float, cfg_scale: float, sampler: str = "dpmpp2m"):
        """The refiner stage: apply_refiner (sdxl_image_generator.py:307-347) -> do_img2img with skip_encode and no added noise
        (sdxl_image_generator_utils.py:986-1016, finish_denoising is always True, sdxl_image_generator.py:566): the base latents
        divided by sqrt(1 + sigma_0^2) of the Img2Img-pruned schedule, then the sampler over that schedule."""
        smp = self.make_sampler(sampler, steps, cfg_scale, z.device, img2img_strength=strength)
        sigmas = smp.discretization(smp.num_steps).to(z.device)
        noised_z = z / torch.sqrt(1.0 + sigmas[0] ** 2.0)
        return self.run_sampler(smp, noised_z, cond, uc)
