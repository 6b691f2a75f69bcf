"""What the SD1.5 samplers (cremage_amd.samplers) and the SDXL samplers (cremage_amd.sgm_hip.sampling) share, and nothing that knows
either model.  A sampling run is a PLAN: the list of its UNet evaluations, built on the CPU from the host fp32 schedule, each with its
sigma, the kind of update that follows it, that update's scalars (Python floats holding the fp32 values of the reference's own torch
expressions on CPU tensors, op for op) and the noise draw it makes.  Here are

  the scalar tables the plans are built from   edm_table, ancestral_table, lms_table, dpmpp2m_multipliers (behaviour of sgm's
                                               sampling.py:165-573 and sampling_utils.py:7-51, which k_diffusion's samplers share)
  the plans both menus run                     plan_heun, plan_euler_a, plan_lms, plan_dpmpp_2s_a, plan_dpmpp_2m
  the two executors and their loop             _TorchSteps (torch arithmetic, one fp32 rounding per reference operation),
                                               _FusedSteps (one input build and one fused HIP step launch per evaluation), run_plan
  the helpers of a fused evaluation            doubled_input, with_time_rows

The fused executor asks the model for an EVALUATOR, `model.fused_evals(ev, x)`, built once per run from the evaluation sigmas `ev`
(CPU fp32, in call order): `evals(k, xin)` runs the network for evaluation k on input `xin` [b, ...] and returns (eps2 contiguous
[2b, ...] with the unconditional half first, c_out); `evals.cfg` is the guidance scale.  samplers._CompVisEvals and
sgm_hip.sampling._DiscreteEvals are the two."""
from __future__ import annotations

import functools

import numpy as np
import torch

from . import knobs, ops


def append_zero(x):
    """x followed by one 0 (the terminal sigma of every k-diffusion schedule)."""
    out = x.new_zeros(x.shape[0] + 1)
    out[:-1] = x
    return out


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


# ------------------------------------------------------------------------------------------------------------------------------
# scalar tables

def _t_fn(sigma):
    return sigma.log().neg()  # sampling_utils.py:46-47


def _sigma_fn(t):
    return t.neg().exp()  # sampling_utils.py:50-51


def dpmpp2m_multipliers(sigmas: torch.Tensor):
    """Per step i of a DPM++ 2M run over the CPU fp32 schedule `sigmas`: (m1, m2, m3, m4, advanced) as Python floats holding fp32
    values.  The arithmetic is DPMPP2MSampler.get_variables / get_mult (sampling.py:460-486) op for op in fp32 torch on the CPU, so
    the scalars equal those of a CPU run of the reference bit for bit.  m3 / m4 are None on the first step; `advanced` is False on the
    first step and on a step whose next sigma is 0 (sampling.py:539-548)."""
    sigmas = sigmas.detach().to("cpu", torch.float32)
    out = []
    for i in range(len(sigmas) - 1):
        sigma, next_sigma = sigmas[i:i + 1], sigmas[i + 1:i + 2]
        t, t_next = _t_fn(sigma), _t_fn(next_sigma)
        h = t_next - t
        m1 = _sigma_fn(t_next) / _sigma_fn(t)
        m2 = (-h).expm1()
        m3 = m4 = None
        if i > 0:
            r = (t - _t_fn(sigmas[i - 1:i])) / h
            m3, m4 = float(1 + 1 / (2 * r)), float(1 / (2 * r))
        out.append((float(m1), float(m2), m3, m4, i > 0 and float(next_sigma) > 0.0))
    return out


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
            t, t_next = _t_fn(sigma), _t_fn(down)   # get_variables
            h = t_next - t
            s = t + 0.5 * h
            m = [float(v[0]) for v in (_sigma_fn(s) / _sigma_fn(t), (-0.5 * h).expm1(), _sigma_fn(t_next) / _sigma_fn(t), (-h).expm1())]
            s_sigma = float(_sigma_fn(s)[0])
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


# ------------------------------------------------------------------------------------------------------------------------------
# plans.  The five below serve both menus: k_diffusion's and sgm's samplers of these names state the same updates.  `b` is the batch
# size of the tables' [b] vectors (their `sum(next) < 1e-14` tests depend on it); `sgm=True` makes the noise draws sgm's.

def _entry(sigma, kind, draw=None, **scalars):
    """One UNet evaluation of a plan: its sigma, the update kind that consumes it, (sigma, sigma_next) of the noise draw made with it
    (None: no draw) and the kind's scalars.  `tick`: a torch.randn_like draw the reference makes here and throws away.  `churn`: the
    std of EDM churn noise (times `s_noise`) drawn and added to x before the evaluation."""
    return dict(sigma=float(sigma), kind=kind, draw=None if draw is None else (float(draw[0]), float(draw[1])), **scalars)


def plan_draws(plan) -> int:
    """How often a run of the plan calls its noise sampler."""
    return sum(1 for e in plan if e["draw"] is not None)


def plan_heun(sh, eta=1., s_noise=1., b=1, s_churn=0., s_tmin=0., s_tmax=float("inf"), sgm=False):
    """sample_heun with churn 0 (k_diffusion sampling.py:166-192: sigma_hat == sigma, and every step ticks for its unused
    torch.randn_like draw, :173), or sgm's HeunEDMSampler (sampling.py:147-219, :321-358), which draws where gamma > 0 only."""
    plan = []
    for r in edm_table(sh, b, s_churn, s_tmin, s_tmax):
        plan.append(_entry(r["sigma_hat"], "heun_1", dt=r["dt"], one_call=not r["two_call"], tick=not sgm, churn=r["churn"], s_noise=s_noise))
        if r["two_call"]:
            plan.append(_entry(r["next"], "heun_2", dt=r["dt"]))
    return plan


def _ancestral_noise(r, s_noise, sgm):
    """The noise of an ancestral step, for its last entry: a draw when the next sigma is not 0.  sgm's AncestralSampler draws on the
    step to sigma 0 as well and throws that one away (sampling.py:222-268): a tick."""
    noisy = r["next"] > 0
    return dict(draw=(r["sigma"], r["next"]) if noisy else None, sigma_up=r["sigma_up"], s_noise=s_noise, tick=sgm and not noisy)


def plan_euler_a(sh, eta=1., s_noise=1., b=1, sgm=False):
    """sgm's EulerAncestralSampler (sampling.py:361-381): an Euler step to sigma_down, then noise of std sigma_up."""
    return [_entry(r["sigma"], "euler_a", dt=r["dt"], **_ancestral_noise(r, s_noise, sgm))
            for r in ancestral_table(sh, b, eta, multipliers=False)]


def plan_dpmpp_2s_a(sh, eta=1., s_noise=1., b=1, sgm=False):
    """sample_dpmpp_2s_ancestral (k_diffusion sampling.py:516-547) / DPMPP2SAncestralSampler (sgm sampling.py:384-456): a second
    evaluation at the midpoint sigma to_sigma(s), then noise of std sigma_up; a step whose sigma_down is 0 is one Euler step."""
    plan = []
    for r in ancestral_table(sh, b, eta):
        noisy = _ancestral_noise(r, s_noise, sgm)
        if not r["two_call"]:
            plan.append(_entry(r["sigma"], "dpmpp2s_1", dt=r["dt"], one_call=True, **noisy))
            continue
        plan.append(_entry(r["sigma"], "dpmpp2s_1", m=r["m"], one_call=False))
        plan.append(_entry(r["s_sigma"], "dpmpp2s_2", m=r["m"], **noisy))
    return plan


def plan_lms(sh, eta=1., s_noise=1., order=4):
    """sample_lms (k_diffusion sampling.py:268-285, order 4) / LinearMultistepSampler (sgm sampling.py:271-306); coefficients: lms_table."""
    return [_entry(sh[i], "lms", coef=list(coef)) for i, coef in enumerate(lms_table(sh, order))]


def plan_dpmpp_2m(sh, eta=1., s_noise=1.):
    """sample_dpmpp_2m (k_diffusion sampling.py:592-615) / DPMPP2MSampler (sgm sampling.py:459-573); multipliers: dpmpp2m_multipliers."""
    return [_entry(sh[i], "dpmpp2m", m=[m1, m2, 0. if m3 is None else m3, 0. if m4 is None else m4], advanced=bool(adv))
            for i, (m1, m2, m3, m4, adv) in enumerate(dpmpp2m_multipliers(sh))]


# ------------------------------------------------------------------------------------------------------------------------------
# helpers of a fused evaluation

def doubled_input(x, c_in=None):
    """cat([x] * 2) * c_in ([2b, ...], contiguous) in ONE elementwise launch; `c_in` a 0-dim device tensor, or None for a plain copy."""
    xx = torch.empty((2,) + tuple(x.shape), dtype=x.dtype, device=x.device)
    src = x.unsqueeze(0).expand_as(xx)
    if c_in is None:
        xx.copy_(src)
    else:
        torch.mul(src, c_in, out=xx)
    return xx.view((2 * x.shape[0],) + tuple(x.shape[1:]))


def with_time_rows(unet, t_rep):
    """The per-step rows of the timestep table `t_rep` [S, N] as a list, each carrying the UNet's hoisted timestep work
    (`UNetModel.time_rows` for the whole table, `ops.attach_time_rows` per row) when `unet` offers it; plain rows otherwise."""
    rows = [t_rep[i] for i in range(t_rep.shape[0])]
    f = getattr(unet, "time_rows", None)
    if f is not None and t_rep.is_cuda and knobs.TIME_ROWS:
        tr = f(t_rep)
        for i, r in enumerate(rows):
            ops.attach_time_rows(r, tr[i], unet)
    return rows


# ------------------------------------------------------------------------------------------------------------------------------
# executors

def _add_noise(x, z, e):
    return x + z * e["s_noise"] * e["sigma_up"]


def _div(a, v: float):
    """a / v as the reference divides: by a 0-dim tensor on a's device, a correctly rounded division.  With a Python number (or a
    0-dim CPU tensor) as the divisor PyTorch's device kernel multiplies by the reciprocal, which differs in the last bit."""
    return a / torch.full((), v, dtype=a.dtype, device=a.device)


_SECOND = ("heun_2", "dpm2_2", "dpmpp2s_2")  # the kinds whose evaluation runs on x2, the first evaluation's trial point


class _TorchSteps:
    """A plan's updates in torch arithmetic, one fp32 rounding per reference operation: any device, any denoiser `model(x, sigma)`."""

    def __init__(self, model, x):
        self.model, self.x = model, x
        self.x2 = self.d = None
        self.hist = []  # LMS: derivatives, the multistep samplers: denoised values; newest first

    def step(self, k, e, z):
        xin = self.x2 if e["kind"] in _SECOND else self.x
        den = self.model(xin, torch.full((xin.shape[0],), e["sigma"], dtype=torch.float32, device=xin.device))
        getattr(self, "_" + e["kind"])(e, den, z)

    def _euler_a(self, e, den, z):
        self.x = self.x + _div(self.x - den, e["sigma"]) * e["dt"]
        if z is not None:
            self.x = _add_noise(self.x, z, e)

    def _heun_1(self, e, den, z):
        d = _div(self.x - den, e["sigma"])
        x2 = self.x + d * e["dt"]
        if e["one_call"]:
            self.x = x2
        else:
            self.x2, self.d = x2, d

    def _heun_2(self, e, den, z):
        d2 = _div(self.x2 - den, e["sigma"])
        self.x = self.x + ((self.d + d2) / 2) * e["dt"]

    def _dpm2_2(self, e, den, z):
        d2 = _div(self.x2 - den, e["sigma"])
        self.x = self.x + d2 * e["dt"]
        if z is not None:
            self.x = _add_noise(self.x, z, e)

    def _lms(self, e, den, z):
        self.hist = [_div(self.x - den, e["sigma"])] + self.hist[:len(e["coef"]) - 1]
        self.x = self.x + sum(c * d for c, d in zip(e["coef"], self.hist))

    def _dpmpp2s_1(self, e, den, z):
        if e["one_call"]:
            return self._euler_a(e, den, z)
        self.x2 = e["m"][0] * self.x - e["m"][1] * den

    def _dpmpp2s_2(self, e, den, z):
        self.x = e["m"][2] * self.x - e["m"][3] * den
        if z is not None:
            self.x = _add_noise(self.x, z, e)

    def _sde_1(self, e, den, z):
        self.x2 = _add_noise(e["m"][0] * self.x - e["m"][1] * den, z, e)

    def _dpmpp2m(self, e, den, z):
        m1, m2, m3, m4 = e["m"]
        self.x = m1 * self.x - m2 * ((m3 * den - m4 * self.hist[0]) if e["advanced"] else den)
        self.hist = [den]

    def _multistep(self, e, den, z, x):
        if z is not None:
            x = x + z * e["p"][0] * e["p"][1] * e["s_noise"]
        self.x, self.hist = x, [den] + self.hist[:1]

    def _sde_2m(self, e, den, z):
        if e["last"]:
            return self._multistep(e, den, None, den)
        x = e["a"] * self.x + e["c1"] * den
        if e["have_old"]:
            x = x + e["c2"] * (den - self.hist[0])
        self._multistep(e, den, z, x)

    def _sde_3m(self, e, den, z):
        if e["last"]:
            return self._multistep(e, den, None, den)
        x = e["a"] * self.x + e["c1"] * den
        if e["order"] == 2:
            x = x + e["phi2"] * _div(den - self.hist[0], e["r"][0])
        elif e["order"] == 3:
            r0, r1 = e["r"]
            d1_0, d1_1 = _div(den - self.hist[0], r0), _div(self.hist[0] - self.hist[1], r1)
            d1 = d1_0 + _div((d1_0 - d1_1) * r0, e["rsum"])
            d2 = _div(d1_0 - d1_1, e["rsum"])
            x = x + e["phi2"] * d1 - e["phi3"] * d2
        self._multistep(e, den, z, x)


class _FusedSteps:
    """A plan's updates as one fused HIP launch per evaluation (crg_cfg_sampler_step, crg_cfg_dpmpp2m_step, crg_cfg_kstep) around the
    model's evaluator (the module docstring): per evaluation one input build, the network and one step launch.  Works on a copy of x."""

    def __init__(self, model, x, plan):
        self.x = x.clone().contiguous()  # updated in place
        self.evals = model.fused_evals(torch.tensor([e["sigma"] for e in plan], dtype=torch.float32), self.x)
        kinds = {e["kind"] for e in plan}
        self.x2 = torch.empty_like(self.x) if kinds & set(_SECOND) else None
        self.d = torch.empty_like(self.x) if kinds & {"heun_2", "dpm2_2"} else None
        # LMS keeps its derivatives, the multistep samplers their denoised values: as many slots as a step reads plus the one it writes
        n_ring = max((len(e["coef"]) if e["kind"] == "lms" else {"sde_3m": 3, "sde_2m": 2, "dpmpp2m": 1}.get(e["kind"], 0) for e in plan), default=0)
        self.ring, self.n = [torch.empty_like(self.x) for _ in range(n_ring)], 0  # n: multistep evaluations so far

    def step(self, k, e, z):
        eps2, c_out = self.evals(k, self.x2 if e["kind"] in _SECOND else self.x)
        noisy = {} if z is None else dict(noise=z.contiguous(), s_noise=e["s_noise"], add_noise=True)
        getattr(self, "_" + e["kind"])(e, (self.x, eps2, c_out, self.evals.cfg), noisy)

    def _euler_a(self, e, head, noisy):
        ops.cfg_sampler_step_("euler_a", *head, sigma=e["sigma"], dt=e["dt"], sigma_up=e["sigma_up"], **noisy)

    def _heun_1(self, e, head, noisy):
        ops.cfg_sampler_step_("heun_1", *head, sigma=e["sigma"], dt=e["dt"], x2=self.x2, d=self.d, one_call=e["one_call"])

    def _heun_2(self, e, head, noisy):
        ops.cfg_sampler_step_("heun_2", *head, sigma=e["sigma"], dt=e["dt"], x2=self.x2, d=self.d)

    def _dpmpp2s_1(self, e, head, noisy):
        if e["one_call"]:
            ops.cfg_sampler_step_("dpmpp2s_1", *head, sigma=e["sigma"], dt=e["dt"], one_call=True, sigma_up=e["sigma_up"], **noisy)
        else:
            ops.cfg_sampler_step_("dpmpp2s_1", *head, x2=self.x2, m=e["m"])

    def _dpmpp2s_2(self, e, head, noisy):
        ops.cfg_sampler_step_("dpmpp2s_2", *head, x2=self.x2, m=e["m"], sigma_up=e["sigma_up"], **noisy)

    def _lms(self, e, head, noisy):
        n, self.n, r = self.n, self.n + 1, len(self.ring)
        hist = [self.ring[(n - j) % r] for j in range(1, len(e["coef"]))]
        ops.cfg_sampler_step_("lms", *head, sigma=e["sigma"], d=self.ring[n % r], hist=hist, coef=e["coef"])

    def _dpmpp2m(self, e, head, noisy):
        ops.cfg_dpmpp2m_step_(head[0], head[1], self.ring[0], head[2], head[3], *e["m"], e["advanced"])

    def _dpm2_2(self, e, head, noisy):
        ops.cfg_kstep_("dpm2_2", *head, sigma=e["sigma"], dt=e["dt"], x2=self.x2, sigma_up=e["sigma_up"], **noisy)

    def _sde_1(self, e, head, noisy):
        ops.cfg_kstep_("sde_1", *head, x2=self.x2, m=e["m"], sigma_up=e["sigma_up"], **noisy)

    def _multistep(self, e, head, noisy, n_old, **scalars):
        """This step's denoised value goes to the ring slot the step does not read; `n_old` previous ones are handed over, newest first."""
        n, self.n, r = self.n, self.n + 1, len(self.ring)
        ops.cfg_kstep_(e["kind"], *head, den_out=self.ring[n % r], old=[self.ring[(n - j) % r] for j in range(1, n_old + 1)],
                       last=e["last"], **scalars, **noisy)

    def _sde_2m(self, e, head, noisy):
        if e["last"]:
            return self._multistep(e, head, {}, 0)
        self._multistep(e, head, noisy, int(e["have_old"]), a=e["a"], c1=e["c1"], c2=e.get("c2", 0.), p=e.get("p", (0., 0.)),
                        have_old=e["have_old"])

    def _sde_3m(self, e, head, noisy):
        if e["last"]:
            return self._multistep(e, head, {}, 0)
        self._multistep(e, head, noisy, e["order"] - 1, a=e["a"], c1=e["c1"], p=e.get("p", (0., 0.)), r=e.get("r", (0., 0.)),
                        rsum=e.get("rsum", 0.), phi2=e.get("phi2", 0.), phi3=e.get("phi3", 0.), order=e["order"])


@torch.no_grad()
def run_plan(model, x, plan, noise_sampler=None, fused=None):
    """Run a plan from x (not mutated): per evaluation the noise draw it makes - `noise_sampler(sigma, sigma_next)` with 0-dim CPU fp32
    tensors, in the order, number and with the arguments of the reference's own calls; torch.randn_like by default - then the
    evaluation and its update.  `fused`: None = whenever model.fused_step_ok(x), False = the torch executor on `model(x, sigma)`,
    True = the fused executor on `model.fused_evals`."""
    if noise_sampler is None:
        draw = lambda e: torch.randn_like(x)  # noqa: E731
    else:
        draw = lambda e: noise_sampler(torch.tensor(e["draw"][0]), torch.tensor(e["draw"][1]))  # noqa: E731
    if fused is None:
        fused = getattr(model, "fused_step_ok", lambda _x: False)(x)
    ex = _FusedSteps(model, x, plan) if fused else _TorchSteps(model, x)
    for k, e in enumerate(plan):
        if e.get("tick"):
            torch.randn_like(x)  # keeps the global RNG stream where the reference leaves it
        if e.get("churn") is not None:  # out of place: the fused executor goes on in place on the new (contiguous) tensor
            ex.x = ex.x + (torch.randn_like(ex.x) * e["s_noise"]) * e["churn"]
        ex.step(k, e, draw(e) if e["draw"] is not None else None)
    return ex.x
