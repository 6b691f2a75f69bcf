"""Small elementwise ops and the fused classifier-free-guidance sampler steps."""
import ctypes as C
from typing import Optional

import torch

from .. import _lib as L
from ._base import _DT, _act_dt, _call, _is_dense, _need_cuda, _p, _written


def timestep_embedding(t: torch.Tensor, dim: int, dtype: torch.dtype = torch.float32) -> torch.Tensor:
    _need_cuda(t)
    t = t.detach().float().contiguous()
    y = torch.empty((t.shape[0], dim), dtype=dtype, device=t.device)
    _call("crg_timestep_embedding", t, _p(t), _p(y), t.shape[0], dim, _DT[dtype])
    return y


def silu(x: torch.Tensor) -> torch.Tensor:
    _need_cuda(x)
    x = x.contiguous()
    y = torch.empty_like(x)
    _call("crg_silu", x, _p(x), _p(y), x.numel(), _act_dt(x))
    return y


def axpby_(y: torch.Tensor, x: torch.Tensor, a: float, b: float = 1.0) -> torch.Tensor:
    """In place y = a*x + b*y (the same dense layout on both sides: the kernel walks numel() consecutive elements of each)."""
    _need_cuda(x, y)
    if x.shape != y.shape or x.stride() != y.stride() or x.dtype != y.dtype:
        raise L.CrgError("axpby_: operands must agree in shape, strides and dtype")
    if not _is_dense(y):  # equal strides: x is then not dense either
        raise L.CrgError(f"axpby_: operands must be dense (no gaps, no expanded dims), got shape {tuple(y.shape)} with strides {y.stride()}")
    _call("crg_axpby", x, _p(x), _p(y), x.numel(), a, b, _act_dt(x))
    return _written(y)


def _check_step(who: str, tail: str, x: torch.Tensor, eps2: torch.Tensor, optional=(), required=()) -> None:
    """The operand contract of every fused step: contiguous fp32 x [b, ...], eps2 [2b, ...], and side buffers [b, ...] (`required`
    ones, and those of `optional` that are not None).  `who` and `tail` complete the wrapper's own message."""
    _need_cuda(x, eps2, *optional, *required)
    n = x.numel()

    def ok(t, numel):
        return t.dtype == torch.float32 and t.is_contiguous() and t.numel() == numel
    if not (ok(x, n) and ok(eps2, 2 * n) and all(ok(t, n) for t in required) and all(t is None or ok(t, n) for t in optional)):
        raise L.CrgError(f"{who}: contiguous fp32 x [b,...], eps [2b,...] and {tail} expected")


def cfg_euler_step_(x: torch.Tensor, eps2: torch.Tensor, noise: Optional[torch.Tensor], sigma: float, dt: float, cfg_scale: float,
                    noise_scale: float = 0.0) -> torch.Tensor:
    """In-place fused sampler step (crg_cfg_euler_step): x fp32 [b, ...], eps2 fp32 [2b, ...] (uncond half first)."""
    _check_step("cfg_euler_step_", "noise [b,...]", x, eps2, (noise,))
    _call("crg_cfg_euler_step", x, _p(x), _p(eps2), _p(noise), x.numel(), float(sigma), float(dt), float(cfg_scale), float(noise_scale))
    return _written(x)


def cfg_ddim_step_(x: torch.Tensor, eps2: torch.Tensor, noise: Optional[torch.Tensor], cfg_scale: float, sqrt_one_minus_a: float,
                   sqrt_a: float, sqrt_a_prev: float, dir_coef: float, sigma: float) -> torch.Tensor:
    """In-place fused DDIM step (crg_cfg_ddim_step): x fp32 [b, ...], eps2 fp32 [2b, ...] (uncond half first), noise fp32 [b, ...]
    (read only when sigma > 0).  The scalars are the fp32 values p_sample_ddim broadcasts (see include/crg_hip.h)."""
    if sigma == 0.0:
        noise = None
    _check_step("cfg_ddim_step_", "noise [b,...]", x, eps2, (noise,))
    if sigma != 0.0 and noise is None:
        raise L.CrgError("cfg_ddim_step_: sigma > 0 needs a noise tensor")
    _call("crg_cfg_ddim_step", x, _p(x), _p(eps2), _p(noise), x.numel(), float(cfg_scale), float(sqrt_one_minus_a), float(sqrt_a),
          float(sqrt_a_prev), float(dir_coef), float(sigma))
    return _written(x)


def cfg_dpmpp2m_step_(x: torch.Tensor, eps2: torch.Tensor, old_den: torch.Tensor, c_out: float, cfg_scale: float, m1: float, m2: float,
                      m3: float, m4: float, advanced: bool) -> torch.Tensor:
    """In-place fused SDXL DPM++ 2M step (crg_cfg_dpmpp2m_step): x fp32 [b, ...], eps2 fp32 [2b, ...] (the raw network output,
    uncond half first), old_den fp32 [b, ...] (the previous step's denoised value, read only when `advanced`; overwritten with this
    step's).  c_out = -sigma (quantised); m1..m4 the fp32 multipliers of DPMPP2MSampler.get_mult (see include/crg_hip.h)."""
    _check_step("cfg_dpmpp2m_step_", "old_den [b,...]", x, eps2, required=(old_den,))
    _call("crg_cfg_dpmpp2m_step", x, _p(x), _p(eps2), _p(old_den), x.numel(), float(c_out), float(cfg_scale), float(m1), float(m2), float(m3), float(m4), 1 if advanced else 0)
    _written(old_den)
    return _written(x)


STEP_KINDS = {"euler_a": L.STEP_EULER_A, "heun_1": L.STEP_HEUN_1, "heun_2": L.STEP_HEUN_2, "dpmpp2s_1": L.STEP_DPMPP2S_1, "dpmpp2s_2": L.STEP_DPMPP2S_2, "lms": L.STEP_LMS}


def cfg_sampler_step_(kind: str, x: torch.Tensor, eps2: torch.Tensor, c_out: float, cfg_scale: float, sigma: float = 0.0, dt: float = 0.0,
                      x2: Optional[torch.Tensor] = None, d: Optional[torch.Tensor] = None, hist=(), noise: Optional[torch.Tensor] = None,
                      sigma_up: float = 0.0, s_noise: float = 1.0, m=(0.0, 0.0, 0.0, 0.0), coef=(0.0, 0.0, 0.0, 0.0), one_call: bool = False,
                      add_noise: bool = False) -> torch.Tensor:
    """In-place fused k-sampler evaluation step (crg_cfg_sampler_step, one launch): `kind` one of STEP_KINDS; x fp32 [b, ...], eps2
    fp32 [2b, ...] (the raw network output, uncond half first); x2 / d / hist / noise fp32 [b, ...] as the kind reads or writes them
    (see include/crg_hip.h); the scalars are the fp32 values the reference's per-step tensors hold.  Returns x."""
    bufs = [x2, d, noise] + list(hist)
    if kind not in STEP_KINDS or len(hist) > 3:
        raise L.CrgError(f"cfg_sampler_step_: unknown kind {kind!r} or more than 3 history buffers")
    _check_step("cfg_sampler_step_", "[b,...] side buffers", x, eps2, bufs)
    a = L.SamplerStepArgs()
    a.kind, a.n = STEP_KINDS[kind], x.numel()
    a.x, a.eps, a.x2, a.d, a.noise = _p(x), _p(eps2), _p(x2), _p(d), _p(noise)
    for k, t in enumerate(hist):
        a.hist[k] = _p(t)
    a.c_out, a.cfg_scale, a.sigma, a.dt, a.sigma_up, a.s_noise = (float(v) for v in (c_out, cfg_scale, sigma, dt, sigma_up, s_noise))
    m, coef = list(m) + [0.0] * (4 - len(m)), list(coef) + [0.0] * (4 - len(coef))
    for k in range(4):
        a.m[k], a.coef[k] = float(m[k]), float(coef[k])
    a.n_hist, a.one_call, a.add_noise = len(hist), 1 if one_call else 0, 1 if add_noise else 0
    _call("crg_cfg_sampler_step", x, C.byref(a))
    for t in (x2, d):
        if t is not None:
            _written(t)
    return _written(x)


KSTEP_KINDS = {"dpm2_2": L.KSTEP_DPM2_2, "sde_1": L.KSTEP_SDE_1, "sde_2m": L.KSTEP_SDE_2M, "sde_3m": L.KSTEP_SDE_3M}


def cfg_kstep_(kind: str, x: torch.Tensor, eps2: torch.Tensor, c_out: float, cfg_scale: float, sigma: float = 0.0, dt: float = 0.0,
               x2: Optional[torch.Tensor] = None, den_out: Optional[torch.Tensor] = None, old=(), noise: Optional[torch.Tensor] = None,
               sigma_up: float = 0.0, s_noise: float = 1.0, m=(0.0, 0.0), a: float = 0.0, c1: float = 0.0, c2: float = 0.0,
               p=(0.0, 0.0), r=(0.0, 0.0), rsum: float = 0.0, phi2: float = 0.0, phi3: float = 0.0, order: int = 1, last: bool = False,
               have_old: bool = False, add_noise: bool = False) -> torch.Tensor:
    """Fused evaluation step of the SD1.5 k-diffusion samplers (crg_cfg_kstep, one launch): `kind` one of KSTEP_KINDS; x fp32 [b, ...],
    eps2 fp32 [2b, ...] (the raw network output, uncond half first); x2 / den_out / old / noise fp32 [b, ...] as the kind reads or
    writes them (see include/crg_hip.h); the scalars are the fp32 values the reference's per-step tensors hold.  Returns x."""
    bufs = [x2, den_out, noise] + list(old)
    if kind not in KSTEP_KINDS or len(old) > 2:
        raise L.CrgError(f"cfg_kstep_: unknown kind {kind!r} or more than 2 history buffers")
    _check_step("cfg_kstep_", "[b,...] side buffers", x, eps2, bufs)
    k = L.KStepArgs()
    k.kind, k.n = KSTEP_KINDS[kind], x.numel()
    k.x, k.eps, k.x2, k.den_out, k.noise = _p(x), _p(eps2), _p(x2), _p(den_out), _p(noise)
    for j, t in enumerate(old):
        k.old[j] = _p(t)
    k.c_out, k.cfg_scale, k.sigma, k.dt, k.sigma_up, k.s_noise = (float(v) for v in (c_out, cfg_scale, sigma, dt, sigma_up, s_noise))
    k.a, k.c1, k.c2, k.rsum, k.phi2, k.phi3 = (float(v) for v in (a, c1, c2, rsum, phi2, phi3))
    for j in range(2):
        k.m[j], k.p[j], k.r[j] = float(m[j]), float(p[j]), float(r[j])
    k.order, k.last, k.have_old, k.add_noise = int(order), 1 if last else 0, 1 if have_old else 0, 1 if add_noise else 0
    _call("crg_cfg_kstep", x, C.byref(k))
    if kind == "sde_1":  # writes x2 only
        _written(x2)
        return x
    if den_out is not None and kind != "dpm2_2":
        _written(den_out)
    return _written(x)
