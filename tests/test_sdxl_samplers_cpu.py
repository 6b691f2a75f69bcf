"""The rest of Cremage's SDXL sampler menu (HeunEDM, EulerAncestral, DPMPP2SAncestral, LinearMultistep) and the EDM schedule, the
parts that need no GPU: the EDM sigmas alone and wrapped, the per-step scalar tables the samplers steer by, the LMS coefficients, every
sampler's torch loop under an analytic denoiser with recorded noise, the name and option tables, and the ctypes mirror of
crg_sampler_step_args - against fixtures made by the reference's own code (tools/gen_golden_sdxl_samplers.py)."""
import contextlib
import math
import os
import re

import pytest
import torch

from cremage_amd.synth import synth_input
from tests.conftest import REPO, load_golden

OPTION_NAMES = dict(s_churn="sampler_s_churn", s_tmin="sampler_s_tmin", s_tmax="sampler_s_tmax", s_noise="sampler_s_noise",
                    eta="sampler_eta", order="sampler_order")
EDM = dict(discretization_sigma_min=0.0292, discretization_sigma_max=14.6146, discretization_rho=3.0)


def _engine():
    from cremage_amd.sgm_hip.sampling import DiffusionEngine
    return DiffusionEngine(torch.nn.Identity(), torch.nn.Identity())


@contextlib.contextmanager
def recorded_noise(monkeypatch, tag, seed):
    """torch.randn_like(x) -> synth_input(f"{tag}.noise{k}") for the k-th draw, as the fixture generator records it."""
    draws = []

    def fake(x, **kw):
        z = synth_input(f"{tag}.noise{len(draws)}", tuple(x.shape), seed).to(device=x.device, dtype=x.dtype)
        draws.append(tuple(x.shape))
        return z
    with monkeypatch.context() as m:
        m.setattr(torch, "randn_like", fake)
        yield draws


def toy_denoiser(inp, sigma, c):
    """tools/gen_golden_sdxl_samplers.py toy_denoiser."""
    s = sigma.reshape(-1, 1, 1, 1)
    return inp / (1.0 + s ** 2) + c["vector"].reshape(-1, 4, 1, 1) * (s / (1.0 + s))


def test_edm_sigmas_bit_equal():
    from cremage_amd.sgm_hip.sampling import EDMDiscretization, make_discretization, wrap_discretization
    meta, g = load_golden("sdxl_samplers_sched")
    k = meta["strength"]
    for n in meta["steps"]:
        d = make_discretization("edm")  # Cremage's preference defaults
        assert (d.sigma_min, d.sigma_max, d.rho) == (0.0292, 14.6146, 3.0)
        assert torch.equal(d(n), g[f"edm_{n}"]), n
        assert torch.equal(wrap_discretization(make_discretization("EDMDiscretization"), n, img2img_strength=k)(n), g[f"edm_i2i_{n}"]), n
        assert torch.equal(wrap_discretization(make_discretization("edm"), n, stage2strength=k)(n), g[f"edm_t2n_{n}"]), n
    assert torch.equal(EDMDiscretization()(20), g["edm_default_20"])
    assert torch.equal(make_discretization("edm", {"discretization_rho": 7.0, "discretization_sigma_min": 0.002,
                                                   "discretization_sigma_max": 80.0})(20), g["edm_default_20"])


def _same(a, b):
    """bit-equal, NaN where the other is NaN"""
    return a.shape == b.shape and torch.equal(torch.isnan(a), torch.isnan(b)) and torch.equal(a.nan_to_num(0.0), b.nan_to_num(0.0))


@pytest.mark.parametrize("sched", ["legacy", "edm", "edm_t2n"])
def test_scalar_tables_bit_equal(sched):
    """sigma_down / sigma_up (get_ancestral_step), DPM++ 2S's m1..m4 and midpoint sigmas, at eta 1 and 0.5."""
    from cremage_amd.sgm_hip.sampling import ancestral_table
    meta, g = load_golden("sdxl_samplers_sched")
    sig = g[f"sigmas_{sched}"]
    for eta in (1.0, 0.5):
        tag = f"{sched}_eta{int(eta * 10):02d}"
        rows = ancestral_table(sig, meta["b"], eta)
        assert _same(torch.tensor([r["sigma_down"] for r in rows]), g[f"down_{tag}"]), tag
        assert _same(torch.tensor([r["sigma_up"] for r in rows]), g[f"up_{tag}"]), tag
        m = torch.tensor([r["m"] if r["two_call"] else [math.nan] * 4 for r in rows])
        assert _same(m, g[f"m_{tag}"]), tag
        mid = torch.tensor([r["s_sigma"] if r["two_call"] else math.nan for r in rows])
        assert _same(mid, g[f"mid_{tag}"]), tag


@pytest.mark.parametrize("sched", ["legacy", "edm", "edm_t2n"])
def test_lms_coefficients(sched):
    """Gauss-Legendre in float64 against the reference's scipy quad (its integrand runs in float32): within 1e-6 relative."""
    from cremage_amd.sgm_hip.sampling import lms_table
    _, g = load_golden("sdxl_samplers_sched")
    ref = g[f"lms_{sched}"]
    table = lms_table(g[f"sigmas_{sched}"], 4)
    assert len(table) == ref.shape[0]
    for i, coeffs in enumerate(table):
        assert len(coeffs) == min(i + 1, 4)
        for j, c in enumerate(coeffs):
            r = float(ref[i, j])
            assert abs(c - r) <= 1e-6 * abs(r) + 1e-12, (i, j, c, r)
        assert torch.isnan(ref[i, len(coeffs):]).all()


def test_toy_loops_match_reference(monkeypatch):
    """Every sampler's torch loop (CPU) under the toy denoiser, on both schedules, with churn / eta / s_noise / order and both
    wrappers: latents within 1e-6 relative (4e-6 for LMS of order 6), the evaluation sigmas bit-equal and in the same order, the same number of noise draws,
    and the fused path's snapping (snap_to_table) gives the reference's sigma_to_idx."""
    from cremage_amd.sgm_hip.sampling import DiscreteDenoiser, snap_to_table
    meta, g = load_golden("sdxl_samplers_toy")
    eng = _engine()
    table = DiscreteDenoiser().sigmas
    B, steps, cfg = meta["B"], meta["steps"], meta["cfg"]
    c = {"vector": synth_input("toy.cv", (B, 4), meta["seed"])}
    uc = {"vector": synth_input("toy.ucv", (B, 4), meta["seed"])}
    assert torch.equal(synth_input("toy.x0", g["x0"].shape, meta["seed"]), g["x0"])
    for name, (key, disc, over, wrapper) in meta["cases"].items():
        opts = dict({OPTION_NAMES[k]: v for k, v in over.items()}, **(EDM if disc == "edm" else {}))
        wrap = {} if wrapper is None else {"img2img_strength" if wrapper[0] == "i2i" else "stage2strength": wrapper[1]}
        smp = eng.make_sampler(key, steps, cfg, "cpu", discretization="edm" if disc == "edm" else "legacy_ddpm", options=opts, **wrap)
        ev = []

        def rec(inp, sigma, cc):
            ev.append(sigma[0].clone())
            return toy_denoiser(inp, sigma, cc)
        with recorded_noise(monkeypatch, "toy." + name, meta["seed"]) as draws:
            x = smp(rec, g["x0"].clone(), cond=c, uc=uc)
        ref = g["x_" + name]
        # LMS past order 4: six-term sums of large coefficients of both signs amplify the last-bit coefficient differences
        tol = 4e-6 if over.get("order", 4) > 4 else 1e-6
        assert (x - ref).abs().max().item() <= tol * ref.abs().max().item(), name
        assert torch.equal(torch.stack(ev), g["ev_" + name]), name
        assert len(draws) == meta["draws"][name], name
        assert torch.equal(snap_to_table(table, g["ev_" + name]), g["idx_" + name]), name


def test_cremage_names_and_options():
    from cremage_amd.sgm_hip import sampling as S
    expect = {"EulerEDM": "euler_edm", "HeunEDM": "heun_edm", "EulerAncestral": "euler_ancestral", "DPMPP2SAncestral": "dpmpp2s_ancestral",
              "DPMPP2M": "dpmpp2m", "LinearMultistep": "linear_multistep"}
    for name, key in expect.items():
        assert S.sampler_key(name) == S.sampler_key(name + "Sampler") == S.sampler_key(key) == key
    assert set(S.SGM_SAMPLERS) == set(expect.values())
    with pytest.raises(ValueError):
        S.sampler_key("DDIM")
    with pytest.raises(ValueError):
        S.sampler_options({"sampler_churn": 1.0})
    with pytest.raises(ValueError):
        S.make_discretization("karras")
    eng = _engine()
    h = eng.make_sampler("HeunEDMSampler", 10, 5.0, "cpu", options={"sampler_s_churn": 0.5})
    assert isinstance(h, S.HeunEDMSampler) and (h.s_churn, h.s_tmin, h.s_tmax, h.s_noise) == (0.5, 0.0, 999.0, 1.0)
    a = eng.make_sampler("DPMPP2SAncestral", 10, 5.0, "cpu", options={"sampler_eta": 0.25, "sampler_s_noise": 0.5})
    assert isinstance(a, S.DPMPP2SAncestralSampler) and (a.eta, a.s_noise) == (0.25, 0.5)
    e = eng.make_sampler("EulerAncestral", 10, 5.0, "cpu")
    assert isinstance(e, S.EulerAncestralSampler) and (e.eta, e.s_noise) == (1.0, 1.0)
    lms = eng.make_sampler("LinearMultistep", 10, 5.0, "cpu", discretization="edm", options={"sampler_order": 6})
    assert isinstance(lms, S.LinearMultistepSampler) and lms.order == 6 and isinstance(lms.discretization, S.EDMDiscretization)
    assert not lms.fused_ok(torch.zeros(1), (None, None))  # order > 4 runs the torch loop
    assert isinstance(eng.make_sampler("heun_edm", 10, 5.0, "cpu", discretization="EDMDiscretization", img2img_strength=0.3).discretization,
                      S.Img2ImgDiscretizationWrapper)


def test_existing_defaults_unchanged():
    """make_sampler("euler_edm") / ("dpmpp2m") keep the legacy schedule and their behaviour; the schedules they run are the ones of
    before (LegacyDDPMDiscretization)."""
    from cremage_amd.sgm_hip import sampling as S
    eng = _engine()
    for key, cls in (("euler_edm", S.EulerEDMSampler), ("dpmpp2m", S.DPMPP2MSampler)):
        smp = eng.make_sampler(key, 30, 5.0, "cpu")
        assert type(smp) is cls and type(smp.discretization) is S.LegacyDDPMDiscretization
        assert torch.equal(smp.discretization(30), S.LegacyDDPMDiscretization()(30))
    e = eng.make_sampler("euler_edm", 30, 5.0, "cpu")
    assert e.s_churn == 0.0 and e.s_noise == 1.0
    assert type(eng.make_sampler("dpmpp2m", 30, 5.0, "cpu", img2img_strength=0.3).discretization.discretization) is S.LegacyDDPMDiscretization


def test_sampler_step_struct_matches_header():
    """Field order of _lib.SamplerStepArgs == crg_sampler_step_args, and the CRG_STEP_* values."""
    from cremage_amd import _lib
    header = open(os.path.join(REPO, "include", "crg_hip.h")).read()
    body = re.search(r"typedef struct \{((?:(?!typedef struct).)*?)\} crg_sampler_step_args;", header, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            names += [re.findall(r"(\w+)(?:\[\d+\])?$", p.strip())[0] for p in decl.split(",")]
    assert names == [f[0] for f in _lib.SamplerStepArgs._fields_]
    enum = dict(re.findall(r"CRG_STEP_(\w+) = (\d+)", header))
    assert {k: int(v) for k, v in enum.items()} == {"EULER_A": _lib.STEP_EULER_A, "HEUN_1": _lib.STEP_HEUN_1, "HEUN_2": _lib.STEP_HEUN_2,
                                                    "DPMPP2S_1": _lib.STEP_DPMPP2S_1, "DPMPP2S_2": _lib.STEP_DPMPP2S_2,
                                                    "LMS": _lib.STEP_LMS}
    assert "crg_cfg_sampler_step" in _lib.SIGNATURES


def _toy_run(smp, B=2, tag="plan"):
    """The sampler's torch path under the toy denoiser -> (latents, the evaluation sigmas in call order)."""
    c, uc = {"vector": synth_input(tag + ".cv", (B, 4), 5)}, {"vector": synth_input(tag + ".ucv", (B, 4), 5)}
    ev = []

    def rec(inp, sigma, cc):
        ev.append(sigma[0].clone())
        return toy_denoiser(inp, sigma, cc)
    return smp(rec, synth_input(tag + ".x0", (B, 4, 5, 3), 5), cond=c, uc=uc), ev


def test_plan_samplers_run_through_shared_run_plan(monkeypatch):
    """Every SDXL sampler but EulerEDM is one call of the run_plan that the SD1.5 samplers run through as well."""
    from cremage_amd import sampler_plan, samplers
    from cremage_amd.sgm_hip import sampling as S
    assert S.run_plan is sampler_plan.run_plan is samplers.run_plan
    seen = []
    monkeypatch.setattr(S, "run_plan", lambda *a, **k: seen.append(len(a[2])) or sampler_plan.run_plan(*a, **k))
    eng = _engine()
    for key in S.SGM_SAMPLERS:
        del seen[:]
        x, ev = _toy_run(eng.make_sampler(key, 4, 5.0, "cpu"))
        assert torch.isfinite(x).all(), key
        assert seen == ([] if key == "euler_edm" else [len(ev)]), (key, seen)  # one plan entry per evaluation


@pytest.mark.parametrize("s_tmin", [0.0, 1.0])
def test_heun_churn_on_pruned_schedule(monkeypatch, s_tmin):
    """HeunEDM with churn on a Txt2Noisy-pruned EDM schedule, which does not end at 0 (the last step makes two evaluations as well):
    one randn_like draw per step with gamma > 0 and no other, and the evaluation sigmas are edm_table's sigma_hat / next sequence bit
    for bit.  s_tmin 1.0 leaves the last steps without churn."""
    from cremage_amd.sgm_hip.sampling import edm_table
    steps, B, churn = 10, 2, 1.0
    opts = dict(EDM, sampler_s_churn=churn, sampler_s_noise=0.9, sampler_s_tmin=s_tmin)
    smp = _engine().make_sampler("heun_edm", steps, 5.0, "cpu", discretization="edm", options=opts, stage2strength=0.5)
    sh = smp.discretization(steps)
    assert 2 < len(sh) < steps + 1 and sh[-1] > 0
    with_gamma = sum(1 for s in sh[:-1].tolist() if s_tmin <= s <= smp.s_tmax and min(churn / (len(sh) - 1), 2 ** 0.5 - 1) > 0)
    assert with_gamma == (len(sh) - 1 if s_tmin == 0.0 else int((sh[:-1] >= 1.0).sum())) and with_gamma > 0
    with recorded_noise(monkeypatch, "heun.pruned", 5) as draws:
        x, ev = _toy_run(smp, B)
    assert torch.isfinite(x).all()
    assert len(draws) == with_gamma
    rows = edm_table(sh, B, churn, s_tmin, smp.s_tmax)
    assert all(r["two_call"] for r in rows) and sum(r["churn"] is not None for r in rows) == with_gamma
    assert torch.equal(torch.stack(ev), torch.tensor([v for r in rows for v in (r["sigma_hat"], r["next"])], dtype=torch.float32))
