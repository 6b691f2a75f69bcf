"""Sampler loop, CFG wrapper and schedules - these STAY ON PYTORCH by design (BASELINE.json
north_star: "The k_diffusion sampler loop ... stay on PyTorch-ROCm so Cremage's generation-info /
LoRA / ControlNet hooks still attach").  All tensors here are [b, 4, L, L] fp32 latents and scalars;
the per-step cost is the UNet call behind `eps_model`.

Mirrors (behaviour, names and argument meaning):
  DiscreteSchedule / DiscreteEpsDDPMDenoiser / CompVisDenoiser   modules/k_diffusion/external.py:41-147
  LDMWrapperForKDiffusion (CFG batch doubling)                    modules/ldm/models/diffusion/ldm_wrapper_for_k_diffusion.py:20-106
  sample_euler / sample_euler_ancestral / get_ancestral_step      modules/k_diffusion/sampling.py:51-58,118-163
  KDiffusionSamplerBase / EulerSampler / EulerAncestralSampler    modules/ldm/models/diffusion/k_diffusion_samplers.py:63-319
  DDIMSampler.make_schedule / stochastic_encode / decode          modules/ldm/models/diffusion/ddim.py:38-75,615-676

The nine table-driven samplers (KSampler) are PLANS run by cremage_amd.sampler_plan's executors, which the SDXL samplers share; this
file adds the plans only k_diffusion has and the CompVis wrapper's evaluator for the fused executor (_CompVisEvals).
"""
from __future__ import annotations

from typing import Callable, List, Optional

import numpy as np
import torch
from torch import nn

from . import knobs, ops
from .sampler_plan import (EDMDiscretization, _entry, _sigma_fn, _t_fn, append_zero, doubled_input, plan_dpmpp_2m,  # noqa: F401
                           plan_dpmpp_2s_a, plan_draws, plan_heun, plan_lms, run_plan, with_time_rows)


def append_dims(x, target_dims):
    """Per-sample vector -> broadcastable against a tensor of `target_dims` dims (trailing singleton axes)."""
    if x.ndim > target_dims:
        raise ValueError(f"cannot view a {x.ndim}-d tensor as {target_dims}-d")
    return x.reshape(tuple(x.shape) + (1,) * (target_dims - x.ndim))


def make_beta_schedule(schedule="linear", n_timestep=1000, linear_start=0.00085, linear_end=0.012):
    """ldm/modules/diffusionmodules/util.py:21-43 ('linear' is what SD uses)."""
    if schedule != "linear":
        raise ValueError(f"schedule '{schedule}' unknown.")
    betas = torch.linspace(linear_start ** 0.5, linear_end ** 0.5, n_timestep, dtype=torch.float64) ** 2
    return betas.numpy()


def make_alphas_cumprod(n_timestep=1000, linear_start=0.00085, linear_end=0.012) -> torch.Tensor:
    """DDPM.register_schedule ddpm.py:134-186: np.cumprod(1 - betas) stored as an fp32 buffer."""
    betas = make_beta_schedule("linear", n_timestep, linear_start, linear_end)
    return torch.tensor(np.cumprod(1.0 - betas, axis=0), dtype=torch.float32)


class DiscreteSchedule(nn.Module):
    """The sigma table of a discrete-time model and the two maps between sigma and (fractional) timestep.

    Behaviour of k_diffusion `DiscreteSchedule` (external.py:41-84), pinned by tests/golden/schedules.npz; the code is this
    repo's own: one ascending fp32 table `log_sigmas` (a buffer, so `.to(device)` moves it) and linear interpolation in
    log-sigma between neighbouring integer timesteps."""

    def __init__(self, sigmas, quantize):
        super().__init__()
        table = sigmas.detach().clone()
        self.register_buffer("sigmas", table)
        self.register_buffer("log_sigmas", table.log())
        self.quantize = quantize

    sigma_min = property(lambda self: self.sigmas[0])
    sigma_max = property(lambda self: self.sigmas[-1])

    def _blend(self, idx_lo, idx_hi, frac):
        """(1 - frac) * log_sigmas[idx_lo] + frac * log_sigmas[idx_hi], the one interpolation rule both maps share."""
        lo, hi = self.log_sigmas[idx_lo], self.log_sigmas[idx_hi]
        return (1 - frac) * lo + frac * hi

    def t_to_sigma(self, t):
        t = t.float()
        below = t.floor()
        return self._blend(below.long(), t.ceil().long(), t - below).exp()

    def get_sigmas(self, n=None):
        """n sigmas from the table's largest to its smallest timestep (evenly spaced in t), then 0; the whole table reversed
        when n is None."""
        if n is None:
            return append_zero(torch.flip(self.sigmas, dims=(0,)))
        last = self.sigmas.shape[0] - 1
        return append_zero(self.t_to_sigma(torch.linspace(last, 0, n, device=self.sigmas.device)))

    def sigma_to_t(self, sigma, quantize=None):
        if quantize is None:
            quantize = self.quantize
        ls = sigma.log()
        if quantize:  # nearest table entry in log-sigma
            return (ls.reshape(1, -1) - self.log_sigmas.reshape(-1, 1)).abs().argmin(dim=0).reshape(sigma.shape)
        # the table is ascending: the bracketing pair is found by binary search (index of the last entry <= log sigma, clamped
        # so that there is always an upper neighbour); out-of-table sigmas clamp to the end timesteps
        n = self.log_sigmas.shape[0]
        lo = (torch.searchsorted(self.log_sigmas, ls.contiguous(), right=True) - 1).clamp(min=0, max=n - 2)
        a, b = self.log_sigmas[lo], self.log_sigmas[lo + 1]
        frac = ((a - ls) / (a - b)).clamp(0, 1)
        return ((1 - frac) * lo + frac * (lo + 1)).reshape(sigma.shape)


class CompVisDenoiser(DiscreteSchedule):
    """eps-prediction wrapper of a CompVis LatentDiffusion (k_diffusion external.py:87-147): sigma_t = sqrt((1 - a_t) / a_t),
    eps = model.apply_model(x / sqrt(sigma^2 + 1), sigma_to_t(sigma), ...), denoised = x - sigma * eps."""

    def __init__(self, model, quantize=False, device='cpu'):
        acp = model.alphas_cumprod
        super().__init__(((1 - acp) / acp) ** 0.5, quantize)
        self.inner_model = model
        self.sigma_data = 1.

    def get_scalings(self, sigma):
        """(c_out, c_in) of the eps parameterisation."""
        return -sigma, 1 / (sigma ** 2 + self.sigma_data ** 2) ** 0.5

    def get_eps(self, *args, **kwargs):
        return self.inner_model.apply_model(*args, **kwargs)

    def forward(self, input, sigma, **kwargs):
        c_out, c_in = [append_dims(x, input.ndim) for x in self.get_scalings(sigma)]
        x_in = input * c_in
        if getattr(input, "_crg_cfg_dup", False):  # a batch-doubled input stays one under a per-sample scaling of equal sigmas
            x_in._crg_cfg_dup = True
        eps = self.get_eps(x_in, self.sigma_to_t(sigma), **kwargs)
        return input + eps * c_out


class LDMWrapperForKDiffusion(nn.Module):
    """ldm_wrapper_for_k_diffusion.py:20-106: classifier-free guidance by batch doubling, applied to the
    DENOISED outputs of the CompVis wrapper.  The concatenated conditioning is built once and reused
    for every step (the reference rebuilds the same `torch.cat` each step, :67-92), which lets the
    cross-attention K/V cache of cremage_amd.ldm_hip.transformer hit."""

    def __init__(self, compviz_wrapper_model, c, unconditional_conditioning, unconditional_guidance_scale: float):
        super().__init__()
        self.compviz_model = compviz_wrapper_model
        self.alphas_cumprod = compviz_wrapper_model.inner_model.alphas_cumprod
        self.ddpm_num_timesteps = compviz_wrapper_model.inner_model.num_timesteps
        self.c = c
        self.unconditional_conditioning = unconditional_conditioning
        self.unconditional_guidance_scale = unconditional_guidance_scale
        self._c_in = None

    _cat_memo = None  # (c, uc, c_in): one concatenated conditioning per (c, uc) pair across sampler instances, so that the
    #                   modules' K/V cache and a captured hipGraph (keyed on the tensor identity) survive from batch to batch

    def _cat_cond(self):
        m = LDMWrapperForKDiffusion._cat_memo
        if self._c_in is None and m is not None and m[0] is self.c and m[1] is self.unconditional_conditioning \
                and torch.is_tensor(self.c) and m[3] == (self.c._version, self.unconditional_conditioning._version):
            self._c_in = m[2]
        if self._c_in is None:
            c, uc = self.c, self.unconditional_conditioning
            if isinstance(c, dict):
                c_in = cat_cond_dict(c, uc)
            else:
                c_in = {"c_crossattn": [torch.cat([uc, c])]}
                LDMWrapperForKDiffusion._cat_memo = (c, uc, c_in, (c._version, uc._version))
            self._c_in = c_in
        return self._c_in

    def eps_pair(self, x, sigma):
        """The raw eps of the batch-doubled UNet call ([2b, ...], unconditional half first) for the fused sampler step:
        the part of apply_model / CompVisDenoiser.forward before the scalings that crg_cfg_euler_step folds in."""
        cv = self.compviz_model
        x_in = torch.cat([x] * 2)
        sigma_in = torch.cat([sigma] * 2)
        _, c_in = [append_dims(v, x_in.ndim) for v in cv.get_scalings(sigma_in)]
        return cv.get_eps(_mark_dup(x_in * c_in), cv.sigma_to_t(sigma_in), cond=self._cat_cond())

    def eps_tables(self, sigmas):
        """(c_in, t) of the CompVis wrapper for a whole vector of sigmas at once - the same elementwise arithmetic
        CompVisDenoiser.forward (external.py:111-114) performs per step on the batch-expanded sigma, so the values are identical;
        computed once per sampling run they replace ~25 tiny launches per step (scalings, log / searchsorted / blend of sigma_to_t)."""
        cv = self.compviz_model
        sigmas = sigmas.to(cv.log_sigmas.device)  # a CPU schedule worked with the per-step scalars (0-dim broadcast); keep it working
        _, c_in = cv.get_scalings(sigmas)
        return c_in, cv.sigma_to_t(sigmas)

    def step_tables(self, sigmas, b):
        """eps_tables of a run's evaluation sigmas as (c_in [S], the doubled batch's timestep rows): the rows carry the wrapped UNet's
        timestep-only work for the whole table when it offers that (with_time_rows)."""
        c_in, t_all = self.eps_tables(sigmas)
        return c_in, with_time_rows(_unet_of(self.compviz_model.inner_model), t_all.reshape(-1, 1).expand(-1, 2 * b).contiguous())

    def eps_pair_pre(self, x, c_in_i, t_row):
        """eps_pair with the step's scalars taken from step_tables: `c_in_i` a 0-dim device tensor, `t_row` the step's timestep
        already expanded to the doubled batch.  ONE elementwise launch builds cat([x] * 2) * c_in."""
        return self.compviz_model.get_eps(_mark_dup(doubled_input(x, c_in_i)), t_row, cond=self._cat_cond())

    def fused_evals(self, ev, x):
        return _CompVisEvals(self, ev, x)

    def fused_step_ok(self, x) -> bool:
        return (self.unconditional_conditioning is not None and self.unconditional_guidance_scale != 1. and x.is_cuda
                and x.dtype == torch.float32 and isinstance(self.compviz_model, CompVisDenoiser))

    def apply_model(self, x, t, **kwargs):
        uc, scale = self.unconditional_conditioning, self.unconditional_guidance_scale
        if uc is None or scale == 1.:
            return self.compviz_model(x, t, self.c)
        x_in = _mark_dup(torch.cat([x] * 2))
        t_in = torch.cat([t] * 2)
        e_t_uncond, e_t = self.compviz_model(x_in, t_in, cond=self._cat_cond()).chunk(2)
        return e_t_uncond + scale * (e_t - e_t_uncond)

    def forward(self, *args, **kwargs):
        return self.apply_model(*args, **kwargs)


def cat_cond_dict(c: dict, uc: dict) -> dict:
    """The batch-doubled dict conditioning of a CFG call (ddim.py:553-562, ldm_wrapper_for_k_diffusion.py:67-92): cat([uc[k], c[k]]) per
    entry.  A `c_concat` entry whose two halves are ONE tensor object (inpaint.py:244-245 puts the same c_cat in both dicts) is marked
    as batch-doubled (ops.mark_cfg_dup), so that the HIP UNet may share its CFG prefix; equal values in two objects are not marked - the
    mark is a promise of the caller, never inferred from data."""
    assert isinstance(uc, dict)
    c_in = dict()
    for k in c:
        if isinstance(c[k], list):
            c_in[k] = [torch.cat([uc[k][i], c[k][i]]) for i in range(len(c[k]))]
            if k == "c_concat":
                for i, t in enumerate(c_in[k]):
                    if uc[k][i] is c[k][i]:
                        _mark_dup(t)
        else:
            c_in[k] = torch.cat([uc[k], c[k]])
    return c_in


def _mark_dup(x_in):
    """The UNet input built by batch doubling: both halves hold the same latents and timesteps (only the conditioning differs) -
    said to the HIP UNet through a tensor attribute, which survives `apply_model` / `DiffusionWrapper.forward` of the reference's
    container as well (they pass x on untouched, ddpm.py:1034, :1517-1519)."""
    if x_in.is_cuda:
        ops.mark_cfg_dup(x_in)
    return x_in


def _unet_of(ldm):
    """The UNet of a LatentDiffusion-like container (ldm.model.diffusion_model), or None."""
    return getattr(getattr(ldm, "model", None), "diffusion_model", None)


class _CompVisEvals:
    """The fused plan executor's evaluator (sampler_plan) over LDMWrapperForKDiffusion, under the conditions of its fused_step_ok:
    every evaluation sigma of the run goes through eps_tables once and the UNet's timestep work is hoisted over the whole table; per
    evaluation one eps_pair_pre input build (with the CFG mark) and the UNet.  c_out is the exact -sigma (CompVisDenoiser does not
    snap it)."""

    def __init__(self, model, ev, x):
        self.model, self.cfg, self.c_out = model, model.unconditional_guidance_scale, [-v for v in ev.tolist()]
        self.c_in, self.t_rows = model.step_tables(ev, x.shape[0])

    def __call__(self, k, xin):
        return self.model.eps_pair_pre(xin, self.c_in[k], self.t_rows[k]).contiguous(), self.c_out[k]


def to_d(x, sigma, denoised):
    return (x - denoised) / (append_dims(sigma, x.ndim) if torch.is_tensor(sigma) else sigma)


def get_ancestral_step(sigma_from, sigma_to, eta=1.):
    if not eta:
        return sigma_to, 0.
    sigma_up = min(sigma_to, eta * (sigma_to ** 2 * (sigma_from ** 2 - sigma_to ** 2) / sigma_from ** 2) ** 0.5)
    sigma_down = (sigma_to ** 2 - sigma_up ** 2) ** 0.5
    return sigma_down, sigma_up


def default_noise_sampler(x):
    return lambda sigma, sigma_next: torch.randn_like(x)


def _host_sigmas(sigmas, sigmas_host):
    """The schedule as a CPU fp32 tensor for everything that steers the loop (comparisons, the ancestral split, the scalar
    step sizes).  A 0-dim DEVICE tensor in a Python `if` / `min` is a device-to-host copy, i.e. a stream synchronisation per
    step: the host then never runs ahead of the GPU and every step starts with the GPU idle for the host's launch latency
    (measured: 40 syncs and ~15 ms of idle GPU per 300 ms batch).  The samplers pass the CPU copy they computed the schedule
    from; without one the device tensor is copied once, before the loop."""
    return sigmas.detach().float().cpu() if sigmas_host is None else sigmas_host


@torch.no_grad()
def sample_euler(model, x, sigmas, extra_args=None, callback=None, disable=None, s_churn=0., s_tmin=0., s_tmax=float('inf'),
                 s_noise=1., sigmas_host=None):
    """sampling.py:118-143 (Algorithm 2 of Karras et al. 2022), including the per-step randn_like draw
    that keeps the global RNG stream aligned with the reference (:128)."""
    extra_args = {} if extra_args is None else extra_args
    s_in = x.new_ones([x.shape[0]])
    sh = _host_sigmas(sigmas, sigmas_host)
    fused = callback is None and not extra_args and getattr(model, "fused_step_ok", lambda _x: False)(x)
    tables = None
    if fused:
        x = x.clone().contiguous()  # updated in place by the fused step
        if knobs.STEP_TABLES and s_churn == 0. and len(sigmas) > 1:  # sigma_hat == sigma on every step: the wrapper's per-step scalars from one vectorised pass
            tables = model.step_tables(sigmas[:-1], x.shape[0])
    for i in range(len(sigmas) - 1):
        gamma = min(s_churn / (len(sigmas) - 1), 2 ** 0.5 - 1) if s_tmin <= sh[i].item() <= s_tmax else 0.
        eps = torch.randn_like(x) * s_noise
        sigma_hat = sh[i] * (gamma + 1)
        if gamma > 0:
            x = x + eps * ((sigma_hat ** 2 - sh[i] ** 2) ** 0.5).item()
        if fused:  # scalings + guidance + Euler update as one kernel (include/crg_hip.h: crg_cfg_euler_step)
            e2 = model.eps_pair_pre(x, tables[0][i], tables[1][i]) if tables is not None else model.eps_pair(x, (sigmas[i] * (gamma + 1)) * s_in)
            ops.cfg_euler_step_(x, e2.contiguous(), None, sigma_hat.item(), (sh[i + 1] - sigma_hat).item(), model.unconditional_guidance_scale)
            continue
        denoised = model(x, (sigmas[i] * (gamma + 1)) * s_in, **extra_args)
        d = to_d(x, sigma_hat.item(), denoised)
        if callback is not None:
            callback({'x': x, 'i': i, 'sigma': sigmas[i], 'sigma_hat': sigma_hat, 'denoised': denoised})
        dt = (sh[i + 1] - sigma_hat).item()
        x = x + d * dt
    return x


@torch.no_grad()
def sample_euler_ancestral(model, x, sigmas, extra_args=None, callback=None, disable=None, eta=1., s_noise=1., noise_sampler=None,
                           sigmas_host=None):
    """sampling.py:147-163."""
    extra_args = {} if extra_args is None else extra_args
    noise_sampler = default_noise_sampler(x) if noise_sampler is None else noise_sampler
    s_in = x.new_ones([x.shape[0]])
    sh = _host_sigmas(sigmas, sigmas_host)
    fused = callback is None and not extra_args and getattr(model, "fused_step_ok", lambda _x: False)(x)
    if fused:
        x = x.clone().contiguous()  # updated in place by the fused step
        tables = knobs.STEP_TABLES and len(sigmas) > 1
        if tables:
            c_in_all, t_rep = model.step_tables(sigmas[:-1], x.shape[0])
    for i in range(len(sigmas) - 1):
        if fused:  # scalings + guidance + Euler update + ancestral noise as one kernel (crg_cfg_euler_step)
            e2 = model.eps_pair_pre(x, c_in_all[i], t_rep[i]) if tables else model.eps_pair(x, sigmas[i] * s_in)
            sigma_down, sigma_up = get_ancestral_step(sh[i], sh[i + 1], eta=eta)
            noise = noise_sampler(sigmas[i], sigmas[i + 1]).contiguous() if sh[i + 1].item() > 0 else None
            ops.cfg_euler_step_(x, e2.contiguous(), noise, sh[i].item(), (sigma_down - sh[i]).item(), model.unconditional_guidance_scale,
                                s_noise * float(sigma_up))
            continue
        denoised = model(x, sigmas[i] * s_in, **extra_args)
        sigma_down, sigma_up = get_ancestral_step(sh[i], sh[i + 1], eta=eta)   # CPU fp32 scalars: no device round trip
        if callback is not None:
            callback({'x': x, 'i': i, 'sigma': sigmas[i], 'sigma_hat': sigmas[i], 'denoised': denoised})
        d = to_d(x, sh[i].item(), denoised)
        dt = (sigma_down - sh[i]).item()
        x = x + d * dt
        if sh[i + 1].item() > 0:
            x = x + noise_sampler(sigmas[i], sigmas[i + 1]) * s_noise * float(sigma_up)
    return x


class KDiffusionSamplerBase(object):
    """k_diffusion_samplers.py:63-296.  `model` is a LatentDiffusion-like object exposing
    `apply_model(x, t, cond)`, `alphas_cumprod`, `num_timesteps` and `device`."""

    def __init__(self, model, sigma_min=0.0316386, sigma_max=14.5521805, beta_d=19.9, beta_min=0.1, eps_s=1e-3):
        self.ldm_model = model
        self.ddpm_num_timesteps = model.num_timesteps
        assert model.alphas_cumprod.shape[0] == self.ddpm_num_timesteps, 'alphas have to be defined for each timestep'
        self.sigma_min, self.sigma_max = sigma_min, sigma_max
        self.beta_d, self.beta_min, self.eps_s = beta_d, beta_min, eps_s
        self.device = model.device
        self.alphas_cumprod = model.alphas_cumprod.clone().detach().to(torch.float32).to(self.device)
        self.sqrt_alphas_cumprod = self.alphas_cumprod.sqrt()
        self.sqrt_one_minus_alphas_cumprod = (1. - self.alphas_cumprod).sqrt()
        self.noise_sampler = None
        self.callback = None

    def compute_sigmas(self, n: int):
        return None

    def compute_sigmas_host(self, n: int):
        """The same schedule computed on the CPU from a cached CPU copy of alphas_cumprod (fp32, the arithmetic of the
        reference run on a CPU device): steers the sampling loop without touching the device (see _host_sigmas)."""
        acp = self._acp_host()
        sched = DiscreteSchedule(((1 - acp) / acp) ** 0.5, False)
        return sched.get_sigmas(n)

    def _acp_host(self):
        """The model's alphas_cumprod as a CPU fp32 tensor, copied once per version of the buffer."""
        m = self.ldm_model
        acp = m.__dict__.get("_crg_acp_cpu")
        if acp is None or acp[0] != m.alphas_cumprod._version:
            acp = m.__dict__["_crg_acp_cpu"] = (m.alphas_cumprod._version, m.alphas_cumprod.detach().float().cpu())
        return acp[1]

    def encode_scalars(self, t_enc: int, sampling_steps: int):
        """(sqrt(acp_t), sqrt(1 - acp_t)) of stochastic_encode(x0, [t_enc] * b, sampling_steps) as Python floats, from the CPU copy of
        the table with stochastic_encode's own fp32 arithmetic - for ops.upscale_noise, without touching the device."""
        t = int((torch.tensor([t_enc]) * 1000.0 / sampling_steps).long())
        acp = self._acp_host()[t]
        return float(acp.sqrt()), float((1. - acp).sqrt())

    @torch.no_grad()
    def _sample_common_prep(self, S, batch_size, shape, conditioning=None, x0=None, unconditional_guidance_scale=1.,
                            unconditional_conditioning=None, **kwargs):
        C, H, W = shape
        size = (batch_size, C, H, W)
        # the reference ignores x_T for k-diffusion samplers and draws randn unless x0 is given (:165-171)
        self.x = torch.randn(size, device=self.device) if x0 is None else x0
        self.compviz_wrapper_model = CompVisDenoiser(self.ldm_model, False).to(self.device)
        self.ldm_wrapper_model = LDMWrapperForKDiffusion(self.compviz_wrapper_model, conditioning, unconditional_conditioning,
                                                         unconditional_guidance_scale)
        self.sigmas = self.compute_sigmas(S)
        self.sigmas_host = self.compute_sigmas_host(S)
        if "denoising_steps" in kwargs:  # partial denoising (img2img), :188-194
            t = kwargs["denoising_steps"]
            self.sigmas = self.sigmas[-(t + 1):]
            self.sigmas_host = self.sigmas_host[-(t + 1):] if self.sigmas_host is not None else None
            assert self.sigmas.shape[0] == t + 1

    @torch.no_grad()
    def sample(self, S, batch_size, shape, conditioning=None, callback=None, x0=None, x_T=None, eta=0., verbose=True,
               unconditional_guidance_scale=1., unconditional_conditioning=None, **kwargs):
        self.callback = None  # the reference accepts `callback` but never forwards it to k-diffusion (:307)
        self._sample_common_prep(S=S, batch_size=batch_size, shape=shape, conditioning=conditioning, x0=x0,
                                 unconditional_guidance_scale=unconditional_guidance_scale,
                                 unconditional_conditioning=unconditional_conditioning, **kwargs)
        return self.do_sample()

    @torch.no_grad()
    def do_sample(self):
        return self.x, None

    @torch.no_grad()
    def stochastic_encode(self, x0, t, sampling_steps, noise=None):
        """k_diffusion_samplers.py:255-296: forward-diffuse x0 to DDPM step t*1000/sampling_steps."""
        if noise is None:
            noise = torch.randn_like(x0)
        t = (t * 1000.0 / sampling_steps).long()
        ex = lambda a: a.gather(-1, t).reshape(t.shape[0], *((1,) * (x0.ndim - 1)))
        return ex(self.sqrt_alphas_cumprod) * x0 + ex(self.sqrt_one_minus_alphas_cumprod) * noise


class EulerSampler(KDiffusionSamplerBase):
    @torch.no_grad()
    def compute_sigmas(self, n):
        return self.compviz_wrapper_model.get_sigmas(n).to(self.device)

    @torch.no_grad()
    def do_sample(self):
        return sample_euler(self.ldm_wrapper_model, self.x, self.sigmas, sigmas_host=self.sigmas_host), None


class EulerAncestralSampler(KDiffusionSamplerBase):
    @torch.no_grad()
    def compute_sigmas(self, n):
        return self.compviz_wrapper_model.get_sigmas(n).to(self.device)

    @torch.no_grad()
    def do_sample(self):
        return sample_euler_ancestral(self.ldm_wrapper_model, self.x, self.sigmas, noise_sampler=self.noise_sampler,
                                      sigmas_host=self.sigmas_host), None


# ------------------------------------------------------------------------------------------------------------------------------
# The rest of Cremage's SD1.5 sampler menu (cremage/utils/sampler_utils.py:21-34): Heun, DPM2, DPM2 A, LMS, DPM++ 2S A, DPM++ SDE,
# DPM++ 2M, DPM++ 2M SDE, DPM++ 3M SDE (k_diffusion sampling.py:166-285, :516-710 behind k_diffusion_samplers.py:321-411), each a PLAN
# for sampler_plan.run_plan.  Heun, LMS, DPM++ 2S A and DPM++ 2M are sampler_plan's own plans; the others follow.

def get_sigmas_karras(n, sigma_min=0.0316386, sigma_max=14.5521805, rho=7., device='cpu'):
    """The Karras et al. schedule followed by 0 (k_diffusion sampling.py:17-23), computed on the CPU in fp32 whatever `device`, so the
    sigmas equal those of a CPU run of the reference bit for bit; the expression is EDMDiscretization's."""
    return EDMDiscretization(sigma_min, sigma_max, rho)(n, do_append_zero=True, device=device)


def _plan_dpm2(sh, ancestral, eta, s_noise):
    plan = []
    for i in range(len(sh) - 1):
        s, sn = sh[i], sh[i + 1]
        target, up = get_ancestral_step(s, sn, eta=eta) if ancestral else (sn, 0.)
        if target == 0:  # Euler
            plan.append(_entry(s, "heun_1", dt=float(target - s), one_call=True, tick=not ancestral))
            continue
        mid = s.log().lerp(target.log(), 0.5).exp()
        plan.append(_entry(s, "heun_1", dt=float(mid - s), one_call=False, tick=not ancestral))
        plan.append(_entry(mid, "dpm2_2", dt=float(target - s), draw=(s, sn) if ancestral else None, sigma_up=float(up), s_noise=s_noise))
    return plan


def plan_dpm2(sh, eta=1., s_noise=1.):
    """sample_dpm_2 with churn 0 (sampling.py:195-223): an Euler step to the log-midpoint sigma, then the midpoint derivative."""
    return _plan_dpm2(sh, False, eta, s_noise)


def plan_dpm2_a(sh, eta=1., s_noise=1.):
    """sample_dpm_2_ancestral (sampling.py:226-252): DPM2 toward sigma_down; noise on the two-call steps only."""
    return _plan_dpm2(sh, True, eta, s_noise)


def plan_dpmpp_sde(sh, eta=1., s_noise=1., r=0.5):
    """sample_dpmpp_sde (sampling.py:550-589) with r = 1/2: fac = 1, so denoised_d is the second evaluation's value and step 2 is
    DPM++ 2S's second update with the SDE's multipliers.  Both draws of a step start at sigma_fn(t)."""
    plan = []
    for i in range(len(sh) - 1):
        if sh[i + 1] == 0:  # Euler, no noise
            plan.append(_entry(sh[i], "heun_1", dt=float(sh[i + 1] - sh[i]), one_call=True))
            continue
        t, t_next = _t_fn(sh[i]), _t_fn(sh[i + 1])
        h = t_next - t
        s = t + h * r
        sd, su = get_ancestral_step(_sigma_fn(t), _sigma_fn(s), eta)
        s_ = _t_fn(sd)
        plan.append(_entry(sh[i], "sde_1", m=[float(_sigma_fn(s_) / _sigma_fn(t)), float((t - s_).expm1())], sigma_up=float(su),
                           s_noise=s_noise, draw=(_sigma_fn(t), _sigma_fn(s))))
        sd, su = get_ancestral_step(_sigma_fn(t), _sigma_fn(t_next), eta)
        t_next_ = _t_fn(sd)
        plan.append(_entry(_sigma_fn(s), "dpmpp2s_2", m=[0., 0., float(_sigma_fn(t_next_) / _sigma_fn(t)), float((t - t_next_).expm1())],
                           sigma_up=float(su), s_noise=s_noise, draw=(_sigma_fn(t), _sigma_fn(t_next))))
    return plan


def plan_dpmpp_2m_sde(sh, eta=1., s_noise=1.):
    """sample_dpmpp_2m_sde, midpoint solver (sampling.py:618-660).  At ONE step the reference raises UnboundLocalError (its `h` is
    never set); here a run whose first step already goes to sigma 0 returns the denoised value, as its longer runs end."""
    plan, h_last = [], None
    for i in range(len(sh) - 1):
        if sh[i + 1] == 0:
            plan.append(_entry(sh[i], "sde_2m", last=True))
            continue
        t, s = -sh[i].log(), -sh[i + 1].log()
        h = s - t
        eta_h = eta * h
        c1 = (-h - eta_h).expm1().neg()
        e = _entry(sh[i], "sde_2m", last=False, a=float(sh[i + 1] / sh[i] * (-eta_h).exp()), c1=float(c1), have_old=i > 0, s_noise=s_noise)
        if i > 0:
            e["c2"] = float(0.5 * c1 * (1 / (h_last / h)))
        if eta:
            e.update(draw=(float(sh[i]), float(sh[i + 1])), p=[float(sh[i + 1]), float((-2 * eta_h).expm1().neg().sqrt())])
        plan.append(e)
        h_last = h
    return plan


def plan_dpmpp_3m_sde(sh, eta=1., s_noise=1.):
    """sample_dpmpp_3m_sde (sampling.py:663-710): first, second, then third order over the last two denoised values.  One step: as
    plan_dpmpp_2m_sde (the reference raises there), the denoised value."""
    plan, h_1, h_2 = [], None, None
    for i in range(len(sh) - 1):
        if sh[i + 1] == 0:
            plan.append(_entry(sh[i], "sde_3m", last=True))
            continue
        t, s = -sh[i].log(), -sh[i + 1].log()
        h = s - t
        h_eta = h * (eta + 1)
        e = _entry(sh[i], "sde_3m", last=False, a=float(torch.exp(-h_eta)), c1=float((-h_eta).expm1().neg()), order=1, s_noise=s_noise)
        if h_1 is not None:
            phi_2 = h_eta.neg().expm1() / h_eta + 1
            e.update(order=2, r=[float(h_1 / h), 0.], phi2=float(phi_2))
        if h_2 is not None:
            r0, r1 = h_1 / h, h_2 / h
            e.update(order=3, r=[float(r0), float(r1)], rsum=float(r0 + r1), phi3=float(phi_2 / h_eta - 0.5))
        if eta:
            e.update(draw=(float(sh[i]), float(sh[i + 1])), p=[float(sh[i + 1]), float((-2 * h * eta).expm1().neg().sqrt())])
        plan.append(e)
        h_1, h_2 = h, h_1
    return plan


# key -> (plan function, schedule): "model" = CompVisDenoiser.get_sigmas, "karras" = get_sigmas_karras (k_diffusion_samplers.py:321-411)
K_SAMPLERS = {"heun": (plan_heun, "model"), "dpm2": (plan_dpm2, "karras"), "dpm2_a": (plan_dpm2_a, "karras"), "lms": (plan_lms, "model"),
              "dpmpp_2s_a": (plan_dpmpp_2s_a, "karras"), "dpmpp_sde": (plan_dpmpp_sde, "karras"), "dpmpp_2m": (plan_dpmpp_2m, "karras"),
              "dpmpp_2m_sde": (plan_dpmpp_2m_sde, "karras"), "dpmpp_3m_sde": (plan_dpmpp_3m_sde, "karras")}
K_SAMPLER_KEYS = tuple(K_SAMPLERS)
# Cremage's SD1.5 sampler menu (cremage/utils/sampler_utils.py:21-34) -> keys
CREMAGE_SD15_SAMPLER_KEYS = {"DDIM": "ddim", "Euler": "euler", "Euler A": "euler_a", "Heun": "heun", "DPM2": "dpm2", "DPM2 A": "dpm2_a",
                             "LMS": "lms", "DPM++ 2S A": "dpmpp_2s_a", "DPM++ SDE": "dpmpp_sde", "DPM++ 2M": "dpmpp_2m",
                             "DPM++ 2M SDE": "dpmpp_2m_sde", "DPM++ 3M SDE": "dpmpp_3m_sde"}


def sampler_key(name: str) -> str:
    """A sampler key, or Cremage's menu name for it ("DPM++ 2M SDE", ...), -> the key."""
    key = CREMAGE_SD15_SAMPLER_KEYS.get(name, name)
    if key not in CREMAGE_SD15_SAMPLER_KEYS.values():
        raise ValueError(f"unknown SD1.5 sampler {name!r} (one of {list(CREMAGE_SD15_SAMPLER_KEYS)} or {list(CREMAGE_SD15_SAMPLER_KEYS.values())})")
    return key


def build_plan(key: str, sigmas_host, eta=1., s_noise=1.):
    """The plan of sampler `key` over the host schedule (CPU fp32, ending in 0)."""
    return K_SAMPLERS[key][0](sigmas_host.detach().to("cpu", torch.float32), eta=eta, s_noise=s_noise)


class BrownianPairNoise:
    """Default noise of DPM++ SDE, whose two draws of a step cover overlapping sigma intervals that start at the same sigma: the
    increments of ONE Brownian motion over [sigma_i, sigma_s] and [sigma_i, sigma_next], each divided by the root of its length, are
    unit Gaussians with correlation rho = sqrt((sigma_i - sigma_s) / (sigma_i - sigma_next)).  A call that starts where the previous
    one started and reaches further returns rho * z1 + sqrt(1 - rho^2) * z'; any other call a fresh draw.  The joint distribution is
    that of the reference's BrownianTreeNoiseSampler; its torchsde random stream is not reproduced.  `generators`: one per image."""

    def __init__(self, shape, device, dtype=torch.float32, generators=None):
        self.shape, self.device, self.dtype, self.generators = tuple(shape), device, dtype, generators
        self.prev = None  # (start sigma, end sigma, z)

    def draw(self):
        if self.generators is not None:
            return torch.stack([torch.randn(self.shape[1:], generator=g, device=self.device, dtype=self.dtype) for g in self.generators])
        return torch.randn(self.shape, device=self.device, dtype=self.dtype)

    def __call__(self, sigma, sigma_next):
        s0, s1 = float(sigma), float(sigma_next)
        z = self.draw()
        if self.prev is not None and self.prev[0] == s0 and s1 < self.prev[1] < s0:
            rho2 = (s0 - self.prev[1]) / (s0 - s1)
            z = rho2 ** 0.5 * self.prev[2] + (1.0 - rho2) ** 0.5 * z
        self.prev = (s0, s1, z)
        return z


class KSampler(KDiffusionSamplerBase):
    """The nine table-driven samplers as one class: `key` one of K_SAMPLER_KEYS picks the plan function and the schedule (the model's
    get_sigmas, or Karras with the base class' sigma_min / sigma_max and rho 7).  `sample(denoising_steps=)` and stochastic_encode are
    the base class', so hires-fix and partial denoising work as for Euler.  `noise_sampler` None: torch.randn_like per draw -
    DPM++ 2M SDE / 3M SDE draw once per step over disjoint sigma intervals, which equals the reference's Brownian tree in
    distribution - and BrownianPairNoise for DPM++ SDE.  No sampler here reproduces the reference's torchsde random stream."""

    def __init__(self, model, key, eta=1., s_noise=1., fused=None, **kwargs):
        if key not in K_SAMPLERS:
            raise ValueError(f"unknown k-sampler {key!r} (one of {list(K_SAMPLERS)})")
        super().__init__(model, **kwargs)
        self.key, self.eta, self.s_noise, self.fused = key, eta, s_noise, fused

    def compute_sigmas_host(self, n):
        if K_SAMPLERS[self.key][1] == "karras":
            return get_sigmas_karras(n, self.sigma_min, self.sigma_max)
        return super().compute_sigmas_host(n)

    @torch.no_grad()
    def compute_sigmas(self, n):
        if K_SAMPLERS[self.key][1] == "karras":
            return get_sigmas_karras(n, self.sigma_min, self.sigma_max, device=self.device)
        return self.compviz_wrapper_model.get_sigmas(n).to(self.device)

    def plan(self, n, denoising_steps=None):
        """The plan of an n-step schedule, or of its last `denoising_steps` steps."""
        sh = self.compute_sigmas_host(n)
        return build_plan(self.key, sh if denoising_steps is None else sh[-(denoising_steps + 1):], self.eta, self.s_noise)

    @torch.no_grad()
    def do_sample(self):
        plan = build_plan(self.key, self.sigmas_host, self.eta, self.s_noise)
        ns = self.noise_sampler
        if ns is None and self.key == "dpmpp_sde":
            ns = BrownianPairNoise(self.x.shape, self.x.device, self.x.dtype)
        return run_plan(self.ldm_wrapper_model, self.x, plan, ns, self.fused), None


def make_ddim_timesteps(ddim_discr_method, num_ddim_timesteps, num_ddpm_timesteps, verbose=False):
    """util.py:46-60 ('uniform')."""
    if ddim_discr_method != 'uniform':
        raise NotImplementedError(f'There is no ddim discretization method called "{ddim_discr_method}"')
    c = num_ddpm_timesteps // num_ddim_timesteps
    return np.asarray(list(range(0, num_ddpm_timesteps, c))) + 1


class DDIMSampler(object):
    """ddim.py: make_schedule :38-75, sample / ddim_sampling :78-190 (from x_T, any eta: the inpainting driver runs eta = 1),
    stochastic_encode :615-654, decode :657-676 (eta = 0, the img2img driver), p_sample_ddim :530-612."""

    def __init__(self, model, schedule="linear", **kwargs):
        self.model = model
        self.ddpm_num_timesteps = model.num_timesteps
        self.schedule = schedule

    def make_schedule(self, ddim_num_steps, ddim_discretize="uniform", ddim_eta=0., verbose=False):
        self.ddim_timesteps = make_ddim_timesteps(ddim_discretize, ddim_num_steps, self.ddpm_num_timesteps)
        acp = self.model.alphas_cumprod.detach().float().cpu()
        assert acp.shape[0] == self.ddpm_num_timesteps
        dev = self.model.device
        a = acp[self.ddim_timesteps]
        a_prev = torch.cat([acp[:1], acp[self.ddim_timesteps[:-1]]])
        self.ddim_alphas = a.to(dev)
        self.ddim_alphas_prev = a_prev.to(dev)
        self.ddim_sqrt_one_minus_alphas = (1. - self.ddim_alphas).sqrt()
        if ddim_eta == 0.:
            sig = torch.zeros_like(a)
        else:
            # make_ddim_sampling_parameters (util.py:63-74): eta * sqrt((1 - a_prev) / (1 - a) * (1 - a / a_prev)) in fp64 on the fp32
            # table values, where the reference's `1 - a` is a torch fp32 subtraction; p_sample_ddim then broadcasts it as fp32
            sig = (ddim_eta * torch.sqrt((1. - a_prev.double()) / (1. - a).double() * (1. - a.double() / a_prev.double()))).float()
        self.ddim_sigmas = sig.to(dev)
        # the fp32 scalars p_sample_ddim computes from the tables per step (ddim.py:581-604), for the fused step: torch.full((b,1,1,1),
        # table[index]) -> fp32, then .sqrt(), 1 - a_prev - sigma ** 2 as fp32 tensor arithmetic
        sq1ma = (1. - a).sqrt()
        dir_coef = (1. - a_prev - sig ** 2).sqrt()
        self._step_scalars = [(float(sq1ma[i]), float(a[i].sqrt()), float(a_prev[i].sqrt()), float(dir_coef[i]), float(sig[i]))
                              for i in range(a.shape[0])]

    @torch.no_grad()
    def stochastic_encode(self, x0, t, use_original_steps=False, noise=None):
        assert not use_original_steps
        if noise is None:
            noise = torch.randn_like(x0)
        ex = lambda a: a.gather(-1, t).reshape(t.shape[0], *((1,) * (x0.ndim - 1)))
        return ex(self.ddim_alphas.sqrt()) * x0 + ex(self.ddim_sqrt_one_minus_alphas) * noise

    @torch.no_grad()
    def p_sample_ddim(self, x, c, t, index, unconditional_guidance_scale=1., unconditional_conditioning=None, noise=None):
        """One step of the elementwise chain; `noise` (z of noise_like) is added as sigma_t * z when this step's sigma is not 0."""
        if unconditional_conditioning is None or unconditional_guidance_scale == 1.:
            e_t = self.model.apply_model(x, t, c)
        else:
            x_in = _mark_dup(torch.cat([x] * 2))
            t_in = torch.cat([t] * 2)
            c_in = self._c_in if getattr(self, "_c_in", None) is not None else torch.cat([unconditional_conditioning, c])
            e_t_uncond, e_t = self.model.apply_model(x_in, t_in, c_in).chunk(2)
            e_t = e_t_uncond + unconditional_guidance_scale * (e_t - e_t_uncond)
        a_t, a_prev = self.ddim_alphas[index], self.ddim_alphas_prev[index]
        pred_x0 = (x - self.ddim_sqrt_one_minus_alphas[index] * e_t) / a_t.sqrt()
        sigma = self._step_scalars[index][4] if hasattr(self, "_step_scalars") else 0.
        if sigma == 0.:
            dir_xt = (1. - a_prev).sqrt() * e_t
            return a_prev.sqrt() * pred_x0 + dir_xt, pred_x0
        sigma_t = self.ddim_sigmas[index]
        dir_xt = (1. - a_prev - sigma_t ** 2).sqrt() * e_t
        return a_prev.sqrt() * pred_x0 + dir_xt + sigma_t * noise, pred_x0

    _cat_memo = None  # (leaves, versions, c_in): one doubled conditioning per (c, uc) across sampler runs, so that the modules' K/V cache
    #                   and a captured hipGraph (keyed on the conditioning's identity) survive from batch to batch

    @staticmethod
    def _leaves(cond):
        if isinstance(cond, dict):
            return tuple((k, i, t) for k in sorted(cond) for i, t in enumerate(cond[k] if isinstance(cond[k], list) else [cond[k]]))
        return (("", 0, cond),)

    def _cat_cond(self, c, uc):
        leaves = self._leaves(uc) + self._leaves(c)
        m = DDIMSampler._cat_memo
        if m is not None and len(m[0]) == len(leaves) and all(a[:2] == b[:2] and a[2] is b[2] for a, b in zip(m[0], leaves)) \
                and m[1] == tuple(t._version for _, _, t in leaves):
            return m[2]
        c_in = cat_cond_dict(c, uc) if isinstance(c, dict) else torch.cat([uc, c])
        DDIMSampler._cat_memo = (leaves, tuple(t._version for _, _, t in leaves), c_in)
        return c_in

    def _fused_loop(self, x, time_range, noise, scale):
        """The fused executor of `sample` and `decode` over the descending timesteps `time_range` from x (not mutated), with the doubled
        conditioning in self._c_in: the UNet's timestep work hoisted over the whole range (with_time_rows), then per step one doubled-
        input copy, the UNet and crg_cfg_ddim_step with the step scalars of make_schedule.  `noise(index, x)`: the step's z, or None."""
        x, b = x.clone().contiguous(), x.shape[0]  # updated in place by the fused step
        t_rep = torch.tensor(time_range.copy(), dtype=torch.long).reshape(-1, 1).expand(-1, 2 * b).contiguous().to(x.device)
        for i, t_row in enumerate(with_time_rows(_unet_of(self.model), t_rep)):
            index = len(time_range) - i - 1
            z = noise(index, x)
            e2 = self.model.apply_model(_mark_dup(doubled_input(x)), t_row, self._c_in)
            ops.cfg_ddim_step_(x, e2.contiguous(), z.contiguous() if z is not None else None, scale, *self._step_scalars[index])
        return x

    @torch.no_grad()
    def sample(self, S, batch_size, shape, conditioning=None, callback=None, eta=0., x_T=None, verbose=False,
               unconditional_guidance_scale=1., unconditional_conditioning=None, noise_sampler=None, **kwargs):
        """ddim.py:78-190 (DDIM from x_T over the whole uniform schedule) -> (samples, None).  `conditioning` / `unconditional_conditioning`
        are tensors or dicts ({"c_concat": [...], "c_crossattn": [...]} for the inpainting model).  `noise_sampler(sigma, index)` returns
        the step's z (noise_like, ddim.py:603) - e.g. pipeline.trajectory_noise_sampler; by default torch.randn is drawn on the steps
        whose sigma is not 0.  With CFG on fp32 device latents and no callback, guidance + the DDIM update + the noise term run as ONE
        kernel per step (crg_cfg_ddim_step) and the UNet's timestep work is computed once for the schedule; otherwise the elementwise
        chain of p_sample_ddim runs."""
        if kwargs.get("mask") is not None or kwargs.get("x0") is not None:
            raise NotImplementedError("DDIMSampler.sample: mask / x0 blending is not restated")
        self.make_schedule(ddim_num_steps=S, ddim_eta=eta, verbose=verbose)
        C, H, W = shape
        size = (batch_size, C, H, W)
        dev = self.model.device
        x = torch.randn(size, device=dev) if x_T is None else x_T
        uc, scale = unconditional_conditioning, unconditional_guidance_scale
        guided = uc is not None and scale != 1.
        self._c_in = self._cat_cond(conditioning, uc) if guided else None
        time_range = np.flip(self.ddim_timesteps)
        total = self.ddim_timesteps.shape[0]

        def noise(index, x):
            sigma = self._step_scalars[index][4]
            if sigma == 0.:
                return None
            return noise_sampler(sigma, index) if noise_sampler is not None else torch.randn(size, device=x.device)
        if guided and callback is None and x.is_cuda and x.dtype == torch.float32:
            x = self._fused_loop(x, time_range, noise, scale)
            self._c_in = None
            return x, None
        for i, step in enumerate(time_range):
            index = total - i - 1
            ts = torch.full((batch_size,), int(step), device=x.device, dtype=torch.long)
            x, _ = self.p_sample_ddim(x, conditioning, ts, index=index, unconditional_guidance_scale=scale,
                                      unconditional_conditioning=uc, noise=noise(index, x))
            if callback:
                callback(i)
        self._c_in = None
        return x, None

    @torch.no_grad()
    def decode(self, x_latent, cond, t_start, unconditional_guidance_scale=1.0, unconditional_conditioning=None,
               use_original_steps=False, callback=None):
        """ddim.py:657-676: the last `t_start` steps of the schedule of make_schedule, from x_latent (not mutated).  `cond` /
        `unconditional_conditioning` are tensors, or dicts ({"c_crossattn": [...], "c_concat": [hint]}, the ControlNet img2img of
        image_generator.py:168-190): dicts are doubled once through _cat_cond - a c_concat entry that is ONE object in both dicts gets
        the CFG mark, as in `sample` - and, with CFG on fp32 device latents and no callback, run `sample`'s fused executor: hoisted time
        rows, one doubled-input copy and crg_cfg_ddim_step with the step scalars of make_schedule.  Tensor conditioning keeps the
        elementwise chain of p_sample_ddim op for op (tests/golden/traj_ddim_img2img pins it); moving that route to the fused step is
        a separate change."""
        assert not use_original_steps
        timesteps = self.ddim_timesteps[:t_start]
        time_range = np.flip(timesteps)
        total_steps = timesteps.shape[0]
        uc, scale = unconditional_conditioning, unconditional_guidance_scale
        guided = uc is not None and scale != 1.
        # one concatenated conditioning for the whole decode (K/V cache friendly); same values as ddim.py:553
        self._c_in = None
        if guided:
            self._c_in = self._cat_cond(cond, uc) if isinstance(cond, dict) else torch.cat([uc, cond])
        if guided and isinstance(cond, dict) and callback is None and x_latent.is_cuda and x_latent.dtype == torch.float32:
            # noise_like of a schedule made with eta > 0 (ddim.py:603)
            x = self._fused_loop(x_latent, time_range, lambda index, x: torch.randn_like(x) if self._step_scalars[index][4] != 0. else None,
                                 scale)
            self._c_in = None
            return x
        x_dec = x_latent
        for i, step in enumerate(time_range):
            index = total_steps - i - 1
            ts = torch.full((x_latent.shape[0],), int(step), device=x_latent.device, dtype=torch.long)
            x_dec, _ = self.p_sample_ddim(x_dec, cond, ts, index=index, unconditional_guidance_scale=unconditional_guidance_scale,
                                          unconditional_conditioning=unconditional_conditioning)
            if callback:
                callback(i)
        self._c_in = None
        return x_dec
