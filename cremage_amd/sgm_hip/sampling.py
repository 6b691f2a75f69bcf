"""SDXL denoiser / guider / sampler glue - stays on PyTorch (north_star), behaviour of
modules/sdxl/sgm/modules/diffusionmodules/{denoiser.py:10-75, denoiser_scaling.py:29-37, discretizer.py:17-78,
guiders.py:24-65, sampling.py:29-573, sampling_utils.py:7-51, wrappers.py:24-34} and DiffusionEngine.decode_first_stage
(sgm/models/diffusion.py:118-136).  Tensors here are [b, 4, L, L] latents and per-sample scalars; the per-step cost
is the UNet call."""
from __future__ import annotations

import functools
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


class EDMDiscretization:
    """discretizer.py:28-48 (+ Discretization.__call__ :17-24): the Karras et al. schedule.  Always computed on the CPU in fp32 with
    the reference's torch expression, then moved to `device`, so a run's sigmas equal those of a CPU run of the reference bit for
    bit whatever the device."""

    def __init__(self, sigma_min=0.002, sigma_max=80.0, rho=7.0):
        self.sigma_min = sigma_min
        self.sigma_max = sigma_max
        self.rho = rho

    def get_sigmas(self, n, device="cpu"):
        ramp = torch.linspace(0, 1, n)
        min_inv_rho = self.sigma_min ** (1 / self.rho)
        max_inv_rho = self.sigma_max ** (1 / self.rho)
        sigmas = (max_inv_rho + ramp * (min_inv_rho - max_inv_rho)) ** self.rho
        return sigmas.to(device)

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


def get_ancestral_step(sigma_from, sigma_to, eta=1.0):
    """sampling_utils.py:22-39 (on the CPU fp32 [b] vectors of the schedule)."""
    if not eta:
        return sigma_to, torch.zeros_like(sigma_to)  # the reference returns a Python 0.0 here, which its append_dims rejects
    sigma_up = torch.minimum(sigma_to, eta * (sigma_to ** 2 * (sigma_from ** 2 - sigma_to ** 2) / sigma_from ** 2) ** 0.5)
    sigma_down = (sigma_to ** 2 - sigma_up ** 2) ** 0.5
    return sigma_down, sigma_up


@functools.lru_cache(maxsize=None)
def _gauss_legendre(n: int):
    nodes, weights = np.polynomial.legendre.leggauss(n)
    return tuple(float(v) for v in nodes), tuple(float(v) for v in weights)


def linear_multistep_coeff(order: int, t, i: int, j: int) -> float:
    """sampling_utils.py:7-19 without scipy: the integral of the Lagrange basis polynomial j (degree order - 1) over [t[i], t[i+1]] by
    float64 Gauss-Legendre quadrature with `order` nodes, exact for that degree.  The reference's adaptive scipy.integrate.quad
    evaluates its integrand in float32 (NumPy 2 keeps the float32 schedule's precision), so its coefficients and these differ in the
    last fp32 bits (<= 3e-7 relative)."""
    if order - 1 > i:
        raise ValueError(f"Order {order} too high for step {i}")
    nodes, weights = _gauss_legendre(max(order, 1))
    a, b = float(t[i]), float(t[i + 1])
    half, mid = 0.5 * (b - a), 0.5 * (b + a)
    tj = float(t[i - j])
    tk = [float(t[i - k]) for k in range(order) if k != j]
    total = 0.0
    for x, w in zip(nodes, weights):
        tau = half * x + mid
        prod = 1.0
        for v in tk:
            prod *= (tau - v) / (tj - v)
        total += w * prod
    return half * total


def edm_table(sigmas: torch.Tensor, b: int, s_churn=0.0, s_tmin=0.0, s_tmax=float("inf")):
    """Per step of EDMSampler.__call__ / sampler_step (sampling.py:165-219, :332-358) over the CPU fp32 schedule, with the reference's
    torch expressions on [b] vectors: dicts of Python floats holding fp32 values - sigma_hat, the churn noise's std (None when
    gamma == 0: no draw), dt = next - sigma_hat, next, and two_call (HeunEDM's second evaluation, sum(next) >= 1e-14)."""
    sigmas = sigmas.detach().to("cpu", torch.float32)
    s_in, num = torch.ones([b]), len(sigmas)
    rows = []
    for i in range(num - 1):
        sigma, nxt = s_in * sigmas[i], s_in * sigmas[i + 1]
        gamma = min(s_churn / (num - 1), 2 ** 0.5 - 1) if s_tmin <= sigmas[i] <= s_tmax else 0.0
        sigma_hat = sigma * (gamma + 1.0)
        churn = float(((sigma_hat ** 2 - sigma ** 2) ** 0.5)[0]) if gamma > 0 else None
        rows.append(dict(sigma_hat=float(sigma_hat[0]), churn=churn, dt=float((nxt - sigma_hat)[0]), next=float(nxt[0]),
                         two_call=not bool(torch.sum(nxt) < 1e-14)))
    return rows


def ancestral_table(sigmas: torch.Tensor, b: int, eta=1.0, multipliers: bool = True):
    """Per step of AncestralSampler / DPMPP2SAncestralSampler (sampling.py:222-268, :384-456) over the CPU fp32 schedule, with the
    reference's torch expressions on [b] vectors: sigma, next, sigma_down, sigma_up, dt = sigma_down - sigma, two_call (DPM++ 2S's
    second evaluation, sum(sigma_down) >= 1e-14) and, on a two-call step with `multipliers`, DPM++ 2S's m1..m4 and its second
    evaluation sigma to_sigma(s) (None otherwise)."""
    sigmas = sigmas.detach().to("cpu", torch.float32)
    s_in = torch.ones([b])
    rows = []
    for i in range(len(sigmas) - 1):
        sigma, nxt = s_in * sigmas[i], s_in * sigmas[i + 1]
        down, up = get_ancestral_step(sigma, nxt, eta=eta)
        two_call = not bool(torch.sum(down) < 1e-14)
        m, s_sigma = None, None
        if two_call and multipliers:
            t, t_next = _to_neg_log_sigma(sigma), _to_neg_log_sigma(down)   # get_variables
            h = t_next - t
            s = t + 0.5 * h
            m = [float(v[0]) for v in (_to_sigma(s) / _to_sigma(t), (-0.5 * h).expm1(), _to_sigma(t_next) / _to_sigma(t), (-h).expm1())]
            s_sigma = float(_to_sigma(s)[0])
        rows.append(dict(sigma=float(sigma[0]), next=float(nxt[0]), sigma_down=float(down[0]), sigma_up=float(up[0]),
                         dt=float((down - sigma)[0]), two_call=two_call, m=m, s_sigma=s_sigma))
    return rows


def lms_table(sigmas: torch.Tensor, order: int):
    """Per step of LinearMultistepSampler.__call__ (sampling.py:282-306): the coefficients, newest derivative first."""
    t = sigmas.detach().to("cpu", torch.float32).tolist()
    out = []
    for i in range(len(t) - 1):
        cur = min(i + 1, order)
        out.append([linear_multistep_coeff(cur, t, i, j) for j in range(cur)])
    return out


def snap_to_table(table: torch.Tensor, sigmas: torch.Tensor) -> torch.Tensor:
    """DiscreteDenoiser.sigma_to_idx (denoiser.py:54-56) of every sigma at once, on the CPU: the index of the nearest table entry."""
    return (sigmas - table[:, None]).abs().argmin(dim=0)


class _FusedEvals:
    """The fused path's denoiser inputs for a run's evaluation sigmas `ev` (CPU fp32, in call order): DiscreteDenoiser.sigma_to_idx
    for all of them at once, the snapped sigmas (c_out = -sq), c_in with the per-call path's device arithmetic and the timestep rows."""

    def __init__(self, dd: "DiscreteDenoiser", network, ev: torch.Tensor, x: torch.Tensor, cc: Dict):
        table = dd.sigmas.detach().cpu()
        idx = snap_to_table(table, ev)
        self.sq = [float(v) for v in table[idx]]
        self.c_in = 1 / (table[idx].to(x.device) ** 2 + 1.0) ** 0.5
        self.t_rows = idx.to(x.device).reshape(-1, 1).expand(-1, 2 * x.shape[0]).contiguous()
        self.network, self.cc, self.k = network, cc, 0

    def __call__(self, xin: torch.Tensor):
        """The next evaluation: one input build, the network; returns (eps [2b, ...], c_out)."""
        k, self.k = self.k, self.k + 1
        xx = torch.empty((2,) + tuple(xin.shape), dtype=xin.dtype, device=xin.device)
        torch.mul(xin.unsqueeze(0).expand_as(xx), self.c_in[k], out=xx)
        eps2 = self.network(xx.view((2 * xin.shape[0],) + tuple(xin.shape[1:])), self.t_rows[k], self.cc)
        return eps2.contiguous(), -self.sq[k]


class _KSampler:
    """Shared plumbing of HeunEDM, EulerAncestral, DPM++ 2S ancestral and LMS: the schedule on the CPU (what steers the loop) and on
    the device, prepare_sampling_loop's `x *= sqrt(1 + sigma_0^2)` on a copy, and the choice of path.  Fused path (CUDA fp32 latents,
    VanillaCFG with scale != 1, the engine's denoiser and network as `parts`): per UNet evaluation one input build, the network and
    one crg_cfg_sampler_step launch.  Otherwise the torch loop, which restates the reference and runs on the CPU as well."""

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
        x = x * float(torch.sqrt(1.0 + sh[0] ** 2.0))
        if self.fused_ok(x, parts):
            return self._fused(parts[0], parts[1], x.contiguous(), cond, uc, sh)
        return self._loop(denoiser, x, cond, uc, sh)

    @staticmethod
    def _sig(v: float, x):
        """A [b] sigma vector on x's device holding the fp32 value v (s_in * sigma)."""
        return torch.full((x.shape[0],), v, dtype=torch.float32, device=x.device)

    @staticmethod
    def _to_d(x, sigma, denoised):
        return (x - denoised) / append_dims(sigma, x.ndim)  # sampling_utils.py:42-43


class HeunEDMSampler(_KSampler):
    """sampling.py:147-219,321-358: Heun steps on the EDM ODE, two UNet calls per step (one when the next sigma is 0), with the EDM
    churn (s_churn > 0: noise drawn and added before the first call of the steps where gamma > 0)."""

    def __init__(self, num_steps: int, guider: VanillaCFG, device="cuda", s_churn=0.0, s_tmin=0.0, s_tmax=float("inf"), s_noise=1.0,
                 fused: bool = True):
        super().__init__(num_steps, guider, device, fused)
        self.s_churn, self.s_tmin, self.s_tmax, self.s_noise = s_churn, s_tmin, s_tmax, s_noise

    def _churn(self, x, r):
        if r["churn"] is None:
            return x
        eps = torch.randn_like(x) * self.s_noise
        return x + eps * r["churn"]

    def _loop(self, denoiser, x, cond, uc, sh):
        for r in edm_table(sh, x.shape[0], self.s_churn, self.s_tmin, self.s_tmax):
            x = self._churn(x, r)
            sigma_hat = self._sig(r["sigma_hat"], x)
            denoised = self.denoise(x, denoiser, sigma_hat, cond, uc)
            d = self._to_d(x, sigma_hat, denoised)
            euler_step = x + r["dt"] * d
            if not r["two_call"]:
                x = euler_step
                continue
            nxt = self._sig(r["next"], x)
            denoised = self.denoise(euler_step, denoiser, nxt, cond, uc)
            d_new = self._to_d(euler_step, nxt, denoised)
            d_prime = (d + d_new) / 2.0
            x = x + d_prime * r["dt"]
        return x

    def _fused(self, dd, network, x, cond, uc, sh):
        from .. import ops
        rows = edm_table(sh, x.shape[0], self.s_churn, self.s_tmin, self.s_tmax)
        ev = [v for r in rows for v in ([r["sigma_hat"], r["next"]] if r["two_call"] else [r["sigma_hat"]])]
        evals = _FusedEvals(dd, network, torch.tensor(ev, dtype=torch.float32), x, self.guider.cat_cond(cond, uc))
        x2, d = torch.empty_like(x), torch.empty_like(x)
        cfg = self.guider.scale
        for r in rows:
            x = self._churn(x, r).contiguous()
            eps2, c_out = evals(x)
            ops.cfg_sampler_step_("heun_1", x, eps2, c_out, cfg, sigma=r["sigma_hat"], dt=r["dt"], x2=x2, d=d, one_call=not r["two_call"])
            if r["two_call"]:
                eps2, c_out = evals(x2)
                ops.cfg_sampler_step_("heun_2", x, eps2, c_out, cfg, sigma=r["next"], dt=r["dt"], x2=x2, d=d)
        return x


class _AncestralSampler(_KSampler):
    """sampling.py:222-268: eta, s_noise, and one torch.randn_like(x) per step - the last step's included, which the reference's
    torch.where throws away."""

    def __init__(self, num_steps: int, guider: VanillaCFG, device="cuda", eta=1.0, s_noise=1.0, fused: bool = True):
        super().__init__(num_steps, guider, device, fused)
        self.eta, self.s_noise = eta, s_noise

    def _ancestral_step(self, x, r):
        noise = torch.randn_like(x)
        return x + noise * self.s_noise * r["sigma_up"] if r["next"] > 0.0 else x


class EulerAncestralSampler(_AncestralSampler):
    """sampling.py:361-381: an Euler step to sigma_down, then noise of std sigma_up."""

    def _loop(self, denoiser, x, cond, uc, sh):
        for r in ancestral_table(sh, x.shape[0], self.eta, multipliers=False):
            sigma = self._sig(r["sigma"], x)
            denoised = self.denoise(x, denoiser, sigma, cond, uc)
            x = x + r["dt"] * self._to_d(x, sigma, denoised)
            x = self._ancestral_step(x, r)
        return x

    def _fused(self, dd, network, x, cond, uc, sh):
        from .. import ops
        rows = ancestral_table(sh, x.shape[0], self.eta, multipliers=False)
        evals = _FusedEvals(dd, network, torch.tensor([r["sigma"] for r in rows], dtype=torch.float32), x, self.guider.cat_cond(cond, uc))
        for r in rows:
            eps2, c_out = evals(x)
            noise = torch.randn_like(x)
            ops.cfg_sampler_step_("euler_a", x, eps2, c_out, self.guider.scale, sigma=r["sigma"], dt=r["dt"], noise=noise,
                                  sigma_up=r["sigma_up"], s_noise=self.s_noise, add_noise=r["next"] > 0.0)
        return x


class DPMPP2SAncestralSampler(_AncestralSampler):
    """sampling.py:384-456: DPM++ 2S ancestral - a second UNet call at the midpoint sigma to_sigma(s) (off the denoiser's grid: it is
    snapped for the scalings only), then noise of std sigma_up; a step whose sigma_down is 0 makes one call (the Euler step)."""

    def _loop(self, denoiser, x, cond, uc, sh):
        for r in ancestral_table(sh, x.shape[0], self.eta):
            sigma = self._sig(r["sigma"], x)
            denoised = self.denoise(x, denoiser, sigma, cond, uc)
            if not r["two_call"]:
                x = x + r["dt"] * self._to_d(x, sigma, denoised)
            else:
                m1, m2, m3, m4 = r["m"]
                x2 = m1 * x - m2 * denoised
                denoised2 = self.denoise(x2, denoiser, self._sig(r["s_sigma"], x), cond, uc)
                x = m3 * x - m4 * denoised2
            x = self._ancestral_step(x, r)
        return x

    def _fused(self, dd, network, x, cond, uc, sh):
        from .. import ops
        rows = ancestral_table(sh, x.shape[0], self.eta)
        ev = [v for r in rows for v in ([r["sigma"], r["s_sigma"]] if r["two_call"] else [r["sigma"]])]
        evals = _FusedEvals(dd, network, torch.tensor(ev, dtype=torch.float32), x, self.guider.cat_cond(cond, uc))
        x2 = torch.empty_like(x)
        cfg = self.guider.scale
        for r in rows:
            eps2, c_out = evals(x)
            noisy = dict(sigma_up=r["sigma_up"], s_noise=self.s_noise, add_noise=r["next"] > 0.0)
            if not r["two_call"]:
                ops.cfg_sampler_step_("dpmpp2s_1", x, eps2, c_out, cfg, sigma=r["sigma"], dt=r["dt"], noise=torch.randn_like(x),
                                      one_call=True, **noisy)
                continue
            ops.cfg_sampler_step_("dpmpp2s_1", x, eps2, c_out, cfg, x2=x2, m=r["m"])
            eps2, c_out = evals(x2)
            ops.cfg_sampler_step_("dpmpp2s_2", x, eps2, c_out, cfg, x2=x2, m=r["m"], noise=torch.randn_like(x), **noisy)
        return x


class LinearMultistepSampler(_KSampler):
    """sampling.py:271-306: linear multistep of the given order over the last derivatives (coefficients: lms_table).  The fused path
    keeps the derivatives in a ring of `order` device buffers and covers order <= 4; a larger order runs the torch loop."""

    FUSED_MAX_ORDER = 4

    def __init__(self, num_steps: int, guider: VanillaCFG, device="cuda", order=4, fused: bool = True):
        super().__init__(num_steps, guider, device, fused)
        if int(order) < 1:
            raise ValueError(f"LMS order must be >= 1 (got {order})")
        self.order = int(order)

    def fused_ok(self, x, parts) -> bool:
        return self.order <= self.FUSED_MAX_ORDER and super().fused_ok(x, parts)

    def _loop(self, denoiser, x, cond, uc, sh):
        ds = []
        for i, coeffs in enumerate(lms_table(sh, self.order)):
            sigma = self._sig(float(sh[i]), x)
            denoised = self.denoise(x, denoiser, sigma, cond, uc)
            ds.append(self._to_d(x, sigma, denoised))
            if len(ds) > self.order:
                ds.pop(0)
            x = x + sum(coeff * d for coeff, d in zip(coeffs, reversed(ds)))
        return x

    def _fused(self, dd, network, x, cond, uc, sh):
        from .. import ops
        table = lms_table(sh, self.order)
        evals = _FusedEvals(dd, network, sh[:-1].clone(), x, self.guider.cat_cond(cond, uc))
        ring = [torch.empty_like(x) for _ in range(self.order)]
        for i, coeffs in enumerate(table):
            eps2, c_out = evals(x)
            hist = [ring[(i - k) % self.order] for k in range(1, len(coeffs))]
            ops.cfg_sampler_step_("lms", x, eps2, c_out, self.guider.scale, sigma=float(sh[i]), d=ring[i % self.order], hist=hist,
                                  coef=coeffs)
        return x


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
        if isinstance(smp, (DPMPP2MSampler, _KSampler)):
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
