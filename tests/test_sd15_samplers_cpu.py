"""The rest of Cremage's SD1.5 sampler menu (Heun, DPM2, DPM2 A, LMS, DPM++ 2S A, DPM++ SDE, DPM++ 2M, DPM++ 2M SDE, DPM++ 3M SDE), the
parts that need no GPU: the Karras schedule, the menu's names, the ctypes mirror of crg_kstep_args, every plan run through the torch
executor under an analytic CFG denoiser with recorded noise, and the default noise of DPM++ SDE - against fixtures made by the
reference's own k_diffusion functions (tools/gen_golden_sd15_samplers.py)."""
import os
import re

import pytest
import torch

from cremage_amd.synth import synth_input
from tests.conftest import REPO, load_golden

NOISY = ("dpm2_a", "dpmpp_2s_a", "dpmpp_sde", "dpmpp_2m_sde", "dpmpp_3m_sde")
TOY_CASES = [(k, n) for k in ("heun", "dpm2", "dpm2_a", "lms", "dpmpp_2s_a", "dpmpp_sde", "dpmpp_2m", "dpmpp_2m_sde", "dpmpp_3m_sde")
             for n in (1, 2, 3, 7) if not (n == 1 and k in ("dpmpp_2m_sde", "dpmpp_3m_sde"))]


class Recorded:
    """tools/gen_golden_sd15_samplers.py Recorded: the k-th call returns synth_input(f"{tag}.noise{k}"); the arguments are kept."""

    def __init__(self, tag, shape, seed, device="cpu"):
        self.tag, self.shape, self.seed, self.device, self.calls = tag, tuple(shape), seed, device, []

    def __call__(self, sigma, sigma_next):
        z = synth_input(f"{self.tag}.noise{len(self.calls)}", self.shape, self.seed).to(self.device)
        self.calls.append([float(sigma), float(sigma_next)])
        return z


def same_calls(calls, ref):
    """The noise sampler's (sigma, sigma_next) arguments, in call order, equal the fixture's bit for bit."""
    return torch.equal(torch.tensor(calls, dtype=torch.float32).reshape(-1, 2), ref)


def toy_model(cu, cc, cfg):
    """tools/gen_golden_sd15_samplers.py toy_model."""
    def model(x, sigma):
        s = sigma.reshape(-1, 1, 1, 1)
        eps_u = x * (s / (1.0 + s ** 2)) - cu.reshape(-1, 4, 1, 1) / (1.0 + s)
        u = x * (s / (1.0 + s ** 2))
        eps_c = u / (1.0 + u.abs()) - cc.reshape(-1, 4, 1, 1) / (1.0 + s)
        den_u, den_c = x - s * eps_u, x - s * eps_c
        return den_u + cfg * (den_c - den_u)
    return model


def _toy():
    meta, g = load_golden("sd15_samplers_toy")
    B, seed = meta["B"], meta["seed"]
    model = toy_model(synth_input("sd15toy.cu", (B, 4), seed), synth_input("sd15toy.cc", (B, 4), seed), meta["cfg"])
    return meta, g, model


def test_karras_sigmas_bit_equal():
    from cremage_amd import samplers as S
    meta, g = load_golden("sd15_samplers_sched")
    assert meta["steps"] == [1, 2, 6, 20]
    for n in meta["steps"]:
        got = S.get_sigmas_karras(n, meta["sigma_min"], meta["sigma_max"], rho=meta["rho"])
        assert got.device.type == "cpu" and got.dtype == torch.float32 and torch.equal(got, g[f"karras_{n}"]), n
        assert torch.equal(S.get_sigmas_karras(n), g[f"karras_{n}"]), n  # the defaults are Cremage's sigma_min / sigma_max


def test_karras_samplers_use_the_host_schedule():
    """compute_sigmas_host of a Karras sampler is the fixture's schedule; a model-schedule sampler keeps the base class' one."""
    from cremage_amd import samplers as S
    _, g = load_golden("sd15_samplers_sched")
    model = type("M", (), dict(num_timesteps=1000, alphas_cumprod=S.make_alphas_cumprod(), device="cpu"))()
    assert torch.equal(S.KSampler(model, "dpmpp_2m").compute_sigmas_host(20), g["karras_20"])
    assert torch.equal(S.KSampler(model, "lms").compute_sigmas_host(20), S.EulerSampler(model).compute_sigmas_host(20))
    with pytest.raises(ValueError):
        S.KSampler(model, "euler")


def test_menu_names_resolve():
    from cremage_amd import pipeline as P
    from cremage_amd import samplers as S
    meta, _ = load_golden("sd15_samplers_sched")
    assert len(meta["names"]) == 12 and set(meta["names"]) == set(S.CREMAGE_SD15_SAMPLER_KEYS)
    for name in meta["names"]:
        key = S.sampler_key(name)
        assert key == S.CREMAGE_SD15_SAMPLER_KEYS[name] == S.sampler_key(key)
        if name != "DDIM":
            assert key in P.SAMPLERS and P._sampler(name)[0] == key
    assert S.sampler_key("DDIM") == "ddim"
    assert len(S.K_SAMPLER_KEYS) == 9 and set(S.K_SAMPLER_KEYS) | {"euler", "euler_a"} == set(P.SAMPLERS)
    assert set(S.K_SAMPLER_KEYS) | {"euler", "euler_a", "ddim"} == set(S.CREMAGE_SD15_SAMPLER_KEYS.values())
    with pytest.raises(ValueError) as e:
        S.sampler_key("DPM++ 4M")
    assert "DPM++ 2M SDE" in str(e.value)
    with pytest.raises(ValueError):
        P._sampler("DDIM")


def test_kstep_struct_matches_header():
    """Field order of _lib.KStepArgs == crg_kstep_args, the CRG_KSTEP_* values and ops.KSTEP_KINDS."""
    from cremage_amd import _lib, ops
    header = open(os.path.join(REPO, "include", "crg_hip.h")).read()
    body = re.search(r"typedef struct \{((?:(?!typedef struct).)*?)\} crg_kstep_args;", header, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            names += [re.findall(r"(\w+)(?:\[\d+\])?$", p.strip())[0] for p in decl.split(",")]
    assert names == [f[0] for f in _lib.KStepArgs._fields_]
    enum = {k: int(v) for k, v in re.findall(r"CRG_KSTEP_(\w+) = (\d+)", header)}
    assert enum == {"DPM2_2": _lib.KSTEP_DPM2_2, "SDE_1": _lib.KSTEP_SDE_1, "SDE_2M": _lib.KSTEP_SDE_2M, "SDE_3M": _lib.KSTEP_SDE_3M}
    assert enum == {"DPM2_2": 0, "SDE_1": 1, "SDE_2M": 2, "SDE_3M": 3}
    assert ops.KSTEP_KINDS == {k.lower(): v for k, v in enum.items()}
    assert "crg_cfg_kstep" in _lib.SIGNATURES
    for lib in (_lib.LIB_PATH.replace("libcrg_hip_f16.so", "libcrg_hip.so"), _lib.LIB_PATH.replace("libcrg_hip.so", "libcrg_hip_f16.so")):
        import ctypes
        assert hasattr(ctypes.CDLL(lib), "crg_cfg_kstep"), lib  # exported by the bf16 and the fp16 library


@pytest.mark.parametrize("key,n", TOY_CASES)
def test_toy_loops_match_reference(key, n):
    """Each plan through the torch executor (CPU) under the toy denoiser with recorded noise: latents within 1e-6 of max|ref|, the
    noise sampler called as often, in the order and with the arguments of the reference's calls, and x0 untouched.

    Measured on the CPU that generated the fixture: every case bit-equal except LMS (1.7e-7 at 3 steps, 7.0e-7 at 7: the last bit of
    lms_table's coefficients).  The scalars come from torch's CPU sqrt / log / exp / expm1, whose last bit depends on the CPU family
    (vendor math library dispatch), exactly as in a run of the reference: on the CPU of an MI355X host the well-conditioned cases
    stayed within 8e-7, but 2-step DPM2 A and DPM++ 2S A moved by 1.1e-3 and 3.4e-4 and 7-step DPM2 A and DPM++ SDE by 2.5e-6 and
    1.4e-6 - get_ancestral_step's sigma_down = sqrt(sigma_next^2 - sigma_up^2) cancels to 5e-6 of its terms when sigma >> sigma_next,
    so one ulp of sigma_up moves sigma_down by a percent.  The fixture holds on the CPU family it was generated on."""
    from cremage_amd import samplers as S
    meta, g, model = _toy()
    x0 = g["x0"].clone()
    sig = g[f"sig_{key}_{n}"]
    if S.K_SAMPLERS[key][1] == "karras":
        assert torch.equal(S.get_sigmas_karras(n), sig)
    rec = Recorded(f"sd15toy.{key}.{n}", x0.shape, meta["seed"])
    plan = S.build_plan(key, sig)
    x = S.run_plan(model, x0, plan, rec)
    ref = g[f"x_{key}_{n}"]
    err = (x - ref).abs().max().item() / ref.abs().max().item()
    print(f"\n[toy] {key} {n} steps: max|x - ref| / max|ref| = {err:.3e}")
    assert err <= 1e-6, (key, n, err)
    calls = g[f"calls_{key}_{n}"]
    assert len(rec.calls) == calls.shape[0] == S.plan_draws(plan), (key, n)
    assert key in NOISY or calls.shape[0] == 0
    assert same_calls(rec.calls, calls), (key, n)
    assert torch.equal(x0, g["x0"])


def test_one_step_multistep_sde_returns_denoised():
    """The reference raises UnboundLocalError there (the fixture records it); ours return the denoised value."""
    from cremage_amd import samplers as S
    meta, g, model = _toy()
    assert meta["raises"] == {"dpmpp_2m_sde_1": "UnboundLocalError", "dpmpp_3m_sde_1": "UnboundLocalError"}
    sig = S.get_sigmas_karras(1)
    for key in ("dpmpp_2m_sde", "dpmpp_3m_sde"):
        plan = S.build_plan(key, sig)
        assert len(plan) == 1 and plan[0]["last"] and S.plan_draws(plan) == 0
        x = S.run_plan(model, g["x0"], plan, lambda s, sn: pytest.fail("no draw on a one-step run"))
        assert torch.equal(x, model(g["x0"], sig[0] * torch.ones(2)))


def test_brownian_pair_noise():
    """The second draw of a step is rho * z1 + sqrt(1 - rho^2) * z' with rho = sqrt((s_i - s_s) / (s_i - s_next)); the next step's
    first draw is fresh."""
    from cremage_amd import samplers as S
    shape = (2, 4, 3, 5)
    zs = [synth_input(f"bp.z{k}", shape, 3) for k in range(3)]
    bp = S.BrownianPairNoise(shape, "cpu")
    it = iter(zs)
    bp.draw = lambda: next(it)
    s_i, s_s, s_next = 5.0, 2.5, 1.25
    z1 = bp(torch.tensor(s_i), torch.tensor(s_s))
    z2 = bp(torch.tensor(s_i), torch.tensor(s_next))
    rho = ((s_i - s_s) / (s_i - s_next)) ** 0.5
    assert torch.equal(z1, zs[0])
    assert torch.allclose(z2, rho * zs[0] + (1 - rho ** 2) ** 0.5 * zs[1], rtol=0, atol=1e-6)
    assert torch.equal(bp(torch.tensor(s_next), torch.tensor(0.8)), zs[2])
    # unit variance and the Brownian correlation, from its own draws
    torch.manual_seed(0)
    bp = S.BrownianPairNoise((1, 4, 128, 128), "cpu")
    a, b = bp(s_i, s_s), bp(s_i, s_next)
    assert abs(b.var().item() - 1.0) < 0.03 and abs((a * b).mean().item() - rho) < 0.03
    g1, g2 = torch.Generator().manual_seed(1), torch.Generator().manual_seed(2)
    per_image = S.BrownianPairNoise((2, 4, 3, 5), "cpu", generators=[g1, g2])(s_i, s_s)
    assert torch.equal(per_image[1], torch.randn((4, 3, 5), generator=torch.Generator().manual_seed(2)))


def test_plan_draw_counts_and_dpmpp_sde_arguments():
    """DPM++ SDE calls its noise sampler twice per two-call step, both from sigma_fn(t), first to the midpoint sigma - what
    BrownianPairNoise keys on; the other samplers draw at most once per step."""
    from cremage_amd import samplers as S
    sig = S.get_sigmas_karras(6)
    plan = S.build_plan("dpmpp_sde", sig)
    assert [e["kind"] for e in plan] == ["sde_1", "dpmpp2s_2"] * 5 + ["heun_1"] and S.plan_draws(plan) == 10
    for a, b in zip(plan[0:10:2], plan[1:10:2]):
        assert a["draw"][0] == b["draw"][0] and a["draw"][1] > b["draw"][1] and b["sigma"] == a["draw"][1]
    counts = {k: S.plan_draws(S.build_plan(k, sig)) for k in S.K_SAMPLER_KEYS if k != "dpmpp_sde"}
    assert counts == dict(heun=0, dpm2=0, dpm2_a=5, lms=0, dpmpp_2s_a=5, dpmpp_2m=0, dpmpp_2m_sde=5, dpmpp_3m_sde=5)
