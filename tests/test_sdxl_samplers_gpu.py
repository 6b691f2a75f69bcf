"""The rest of Cremage's SDXL sampler menu on a real MI355X: every kind of crg_cfg_sampler_step against the CPU fp32 chain (with the
buffers a kind must not read filled with NaN), and tiny sgm UNet trajectories of HeunEDM, EulerAncestral, DPM++ 2S ancestral and
LMS on both schedules through the fused and the unfused path, DPM++ 2M on the EDM schedule, an img2img re-entry and a pruned base
stage, against fixtures made by the reference's own modules (tools/gen_golden_sdxl_samplers.py)."""
import ctypes

import pytest
import torch

from cremage_amd.synth import synth_input
from tests.conftest import load_golden, rel_l2
from tests.test_hip_models import DEV, TOL_TRAJ, close
from tests.test_refiner_gpu import _tiny_engine
from tests.test_sdxl_samplers_cpu import recorded_noise

pytestmark = pytest.mark.gpu

SHAPE, CFG = (2, 4, 33, 47), 5.0  # a ragged element count


def _den(eps2, xin, c_out, cfg):
    b = xin.shape[0]
    den_u = eps2[:b] * c_out + xin
    den_c = eps2[b:] * c_out + xin
    return den_u + cfg * (den_c - den_u)


def _t(name, scale=1.0):
    return synth_input("smpk." + name, SHAPE, 7) * scale


def _check(got, ref, what):
    assert torch.isfinite(got).all(), what
    assert (got.cpu() - ref).abs().max().item() <= 1e-6 * ref.abs().max().item(), what


def _dev(*ts):
    return [t.to(DEV).contiguous() for t in ts]


def _nan():
    return torch.full(SHAPE, float("nan"), device=DEV)


def test_sampler_step_euler_a_and_heun():
    from cremage_amd import ops
    x, z, d0 = _t("x", 10.0), _t("z"), _t("d")
    eps2 = synth_input("smpk.e", (2 * SHAPE[0],) + SHAPE[1:], 7)
    sigma, c_out, dt, up, s_noise = 9.5, -9.4, -3.25, 2.5, 0.9
    # EULER_A, with and without noise (a NaN noise tensor is not read when add_noise is off)
    den = _den(eps2, x, c_out, CFG)
    base = x + dt * ((x - den) / sigma)
    for add in (True, False):
        xg, eg, zg = _dev(x, eps2, z)
        ops.cfg_sampler_step_("euler_a", xg, eg, c_out, CFG, sigma=sigma, dt=dt, noise=zg if add else _nan(), sigma_up=up, s_noise=s_noise,
                              add_noise=add)
        _check(xg, base + (z * s_noise) * up if add else base, f"euler_a noise={add}")
    # HEUN_1 two-call: x untouched, x2 and d written
    xg, eg = _dev(x, eps2)
    x2, dg = _nan(), _nan()
    ops.cfg_sampler_step_("heun_1", xg, eg, c_out, CFG, sigma=sigma, dt=dt, x2=x2, d=dg)
    d_ref = (x - den) / sigma
    _check(x2, x + dt * d_ref, "heun_1 x2")
    _check(dg, d_ref, "heun_1 d")
    assert torch.equal(xg.cpu(), x)
    # HEUN_1 one-call: x = the Euler step; x2 / d neither read nor written
    xg, eg = _dev(x, eps2)
    x2, dg = _nan(), _nan()
    ops.cfg_sampler_step_("heun_1", xg, eg, c_out, CFG, sigma=sigma, dt=dt, x2=x2, d=dg, one_call=True)
    _check(xg, x + dt * d_ref, "heun_1 one call")
    assert torch.isnan(x2).all() and torch.isnan(dg).all()
    # HEUN_2
    xin, nxt = x + dt * d_ref, 6.25
    den2 = _den(eps2, xin, -6.2, CFG)
    ref = x + ((d0 + (xin - den2) / nxt) / 2.0) * dt
    xg, eg, x2, dg = _dev(x, eps2, xin, d0)
    ops.cfg_sampler_step_("heun_2", xg, eg, -6.2, CFG, sigma=nxt, dt=dt, x2=x2, d=dg)
    _check(xg, ref, "heun_2")


def test_sampler_step_dpmpp2s():
    from cremage_amd import ops
    x, z, x2h = _t("x", 10.0), _t("z"), _t("x2", 8.0)
    eps2 = synth_input("smpk.e2", (2 * SHAPE[0],) + SHAPE[1:], 7)
    m, c_out, up, s_noise = (0.75, -0.4, 0.55, -0.6), -9.4, 1.5, 1.1
    den = _den(eps2, x, c_out, CFG)
    # first call: x2 = m1 x - m2 den; x untouched
    xg, eg = _dev(x, eps2)
    x2 = _nan()
    ops.cfg_sampler_step_("dpmpp2s_1", xg, eg, c_out, CFG, x2=x2, m=m)
    _check(x2, m[0] * x - m[1] * den, "dpmpp2s_1 x2")
    assert torch.equal(xg.cpu(), x)
    # second call, with and without noise
    den2 = _den(eps2, x2h, -7.0, CFG)
    for add in (True, False):
        xg, eg, x2g, zg = _dev(x, eps2, x2h, z)
        ops.cfg_sampler_step_("dpmpp2s_2", xg, eg, -7.0, CFG, x2=x2g, m=m, noise=zg if add else _nan(), sigma_up=up, s_noise=s_noise,
                              add_noise=add)
        ref = m[2] * x - m[3] * den2
        _check(xg, ref + (z * s_noise) * up if add else ref, f"dpmpp2s_2 noise={add}")
    # one-call step: the Euler step to sigma_down and the noise; x2 not read
    sigma, dt = 9.5, -9.5
    xg, eg, zg = _dev(x, eps2, z)
    ops.cfg_sampler_step_("dpmpp2s_1", xg, eg, c_out, CFG, sigma=sigma, dt=dt, x2=_nan(), noise=zg, sigma_up=up, s_noise=s_noise,
                          one_call=True, add_noise=True)
    _check(xg, (x + dt * ((x - den) / sigma)) + (z * s_noise) * up, "dpmpp2s_1 one call")


def _lms_raw(x, eps2, d, hist_ptrs, n_hist, c_out, sigma, coef):
    """crg_cfg_sampler_step through the struct directly: hist pointers past n_hist set (to NaN buffers) must stay unread."""
    from cremage_amd import _lib as L
    from cremage_amd import ops
    a = L.SamplerStepArgs()
    a.kind, a.n, a.x, a.eps, a.d = L.STEP_LMS, x.numel(), x.data_ptr(), eps2.data_ptr(), d.data_ptr()
    for k, t in enumerate(hist_ptrs):
        a.hist[k] = t.data_ptr()
    a.c_out, a.cfg_scale, a.sigma, a.n_hist = c_out, CFG, sigma, n_hist
    for k, c in enumerate(coef):
        a.coef[k] = c
    h = ops._h(x)
    return L.load().crg_cfg_sampler_step(h, ops._st(), ctypes.byref(a)), h


def test_sampler_step_lms_reads_only_existing_history():
    x = _t("x", 10.0)
    eps2 = synth_input("smpk.e3", (2 * SHAPE[0],) + SHAPE[1:], 7)
    hist = [_t(f"h{k}") for k in range(3)]
    coef = [1.5, -0.75, 0.3125, -0.0625]
    c_out, sigma = -3.1, 3.125
    d_ref = (x - _den(eps2, x, c_out, CFG)) / sigma
    for n_hist in range(4):
        acc = coef[0] * d_ref
        for k in range(n_hist):
            acc = acc + coef[k + 1] * hist[k]
        xg, eg = _dev(x, eps2)
        dg = _nan()
        ptrs = [h.to(DEV) for h in hist[:n_hist]] + [_nan() for _ in range(3 - n_hist)]
        rc, _ = _lms_raw(xg, eg, dg, ptrs, n_hist, c_out, sigma, coef)
        torch.cuda.synchronize()
        assert rc == 0
        _check(xg, x + acc, f"lms n_hist={n_hist}")
        _check(dg, d_ref, f"lms d n_hist={n_hist}")


def test_sampler_step_rejects_bad_arguments():
    from cremage_amd import _lib as L
    from cremage_amd import ops
    x, eps2 = torch.zeros(SHAPE, device=DEV), torch.zeros((2 * SHAPE[0],) + SHAPE[1:], device=DEV)
    for kw, msg in ((dict(kind="euler_a", sigma=0.0), "positive"), (dict(kind="euler_a", sigma=1.0, add_noise=True), "noise"),
                    (dict(kind="heun_1", sigma=1.0), "x2"), (dict(kind="heun_2", sigma=1.0, x2=x.clone()), "needs d"),
                    (dict(kind="lms", sigma=1.0), "needs d"), (dict(kind="dpmpp2s_2", m=(1, 1, 1, 1)), "x2")):
        with pytest.raises(L.CrgError, match=msg):
            ops.cfg_sampler_step_(kw.pop("kind"), x, eps2, -1.0, CFG, **kw)
    rc, h = _lms_raw(x, eps2, x.clone(), [], 4, -1.0, 1.0, [1.0])
    assert rc == -22 and b"n_hist" in L.load().crg_last_error(h)


def _cond(tag, B, seed):
    return ({"crossattn": synth_input(tag + ".c", (B, 77, 128), seed).to(DEV), "vector": synth_input(tag + ".cv", (B, 96), seed).to(DEV)},
            {"crossattn": synth_input(tag + ".uc", (B, 77, 128), seed).to(DEV), "vector": synth_input(tag + ".ucv", (B, 96), seed).to(DEV)})


# the fused launches a step of each sampler makes: (kind, one_call) per UNet evaluation
def _expected_kinds(key, S, t2n=False):
    last_two = t2n   # a pruned schedule does not end at 0: the last step makes two calls as well
    if key == "heun_edm":
        return [("heun_1", False), ("heun_2", False)] * (S - 1) + ([("heun_1", False), ("heun_2", False)] if last_two else [("heun_1", True)])
    if key == "dpmpp2s_ancestral":
        return [("dpmpp2s_1", False), ("dpmpp2s_2", False)] * (S - 1) + ([("dpmpp2s_1", False), ("dpmpp2s_2", False)] if last_two
                                                                         else [("dpmpp2s_1", True)])
    return [({"euler_ancestral": "euler_a", "linear_multistep": "lms"}[key], False)] * S


def _run_both(monkeypatch, eng, tag, seed, run, unfused, expect=None):
    """run() through the fused path (counting crg_cfg_sampler_step launches), then unfused(); both with the recorded noise."""
    from cremage_amd import ops
    calls = []
    real = ops.cfg_sampler_step_
    with monkeypatch.context() as m:
        m.setattr(ops, "cfg_sampler_step_", lambda kind, *a, **k: calls.append((kind, bool(k.get("one_call")))) or real(kind, *a, **k))
        with recorded_noise(monkeypatch, tag, seed) as dr:
            fused = run()
        nf = len(dr)
        with recorded_noise(monkeypatch, tag, seed) as dr:
            unf = unfused()
        nu = len(dr)
    if expect is not None:
        assert calls[:len(expect)] == expect and len(calls) == len(expect), calls
    return fused, unf, nf, nu


@pytest.mark.parametrize("disc", ["legacy", "edm"])
@pytest.mark.parametrize("key", ["heun_edm", "euler_ancestral", "dpmpp2s_ancestral", "linear_multistep"])
def test_sdxl_trajectory_new_samplers(key, disc, monkeypatch):
    """6 steps + decode of each new sampler vs the reference's stack, fused (one crg_cfg_sampler_step per UNet evaluation) and
    unfused, with the reference's noise draws; fused and unfused agree within 1e-5 relative."""
    meta, g = load_golden(f"traj_sdxl_{key}")
    eng = _tiny_engine(meta)
    B, L, S, seed, tag = meta["B"], meta["L"], meta["S"], meta["seed"], f"{key}.{disc}"
    c, uc = _cond(tag, B, seed)
    x0 = synth_input(tag + ".x0", (B, 4, L, L), seed).to(DEV)
    keep = x0.clone()
    dname = "edm" if disc == "edm" else "legacy_ddpm"

    def unfused():
        smp = eng.make_sampler(key, S, meta["cfg"], DEV, discretization=dname)
        smp.fused = False
        return eng.run_sampler(smp, x0, c, uc)
    fused, unf, nf, nu = _run_both(monkeypatch, eng, tag, seed, lambda: eng.sample(x0, c, uc, S, meta["cfg"], sampler=key, discretization=dname),
                                   unfused, _expected_kinds(key, S))
    assert torch.equal(x0, keep)
    assert nf == nu == meta["draws"][disc]
    close(fused, g[f"x_{disc}"], TOL_TRAJ, f"{key} {disc} latent (fused)")
    close(unf, g[f"x_{disc}"], TOL_TRAJ, f"{key} {disc} latent (unfused)")
    assert rel_l2(fused.cpu(), unf.cpu()) <= 1e-5
    img = eng.decode_first_stage(fused)
    assert (img.cpu() - g[f"img_{disc}"]).abs().max().item() < 4e-3


def test_sdxl_trajectory_heun_churn(monkeypatch):
    """HeunEDM with s_churn > 0 (a noise draw and the input-side add before each step's first call)."""
    meta, g = load_golden("traj_sdxl_heun_edm")
    eng = _tiny_engine(meta)
    B, L, S, seed, tag = meta["B"], meta["L"], meta["S"], meta["seed"], "heun_edm.churn"
    c, uc = _cond(tag, B, seed)
    x0 = synth_input(tag + ".x0", (B, 4, L, L), seed).to(DEV)
    opts = {"sampler_s_churn": meta["churn"]["s_churn"], "sampler_s_noise": meta["churn"]["s_noise"]}

    def unfused():
        smp = eng.make_sampler("HeunEDM", S, meta["cfg"], DEV, options=opts)
        smp.fused = False
        return eng.run_sampler(smp, x0, c, uc)
    fused, unf, nf, nu = _run_both(monkeypatch, eng, tag, seed, lambda: eng.sample(x0, c, uc, S, meta["cfg"], sampler="HeunEDM", options=opts),
                                   unfused, _expected_kinds("heun_edm", S))
    assert nf == nu == meta["draws"]["churn"]
    close(fused, g["x_churn"], TOL_TRAJ, "heun churn (fused)")
    close(unf, g["x_churn"], TOL_TRAJ, "heun churn (unfused)")


def test_sdxl_trajectory_dpmpp2m_edm(monkeypatch):
    """DPM++ 2M (crg_cfg_dpmpp2m_step) on the EDM schedule: off-grid sigmas snapped for the scalings only."""
    from cremage_amd import ops
    meta, g = load_golden("traj_sdxl_samplers_extra")
    eng = _tiny_engine(meta)
    B, L, S, seed, tag = meta["B"], meta["L"], meta["S"], meta["seed"], "dpm2m_edm"
    c, uc = _cond(tag, B, seed)
    x0 = synth_input(tag + ".x0", (B, 4, L, L), seed).to(DEV)
    calls = []
    real = ops.cfg_dpmpp2m_step_
    monkeypatch.setattr(ops, "cfg_dpmpp2m_step_", lambda *a: calls.append(a[-1]) or real(*a))
    fused = eng.sample(x0, c, uc, S, meta["cfg"], sampler="DPMPP2M", discretization="edm")
    assert calls == [False] + [True] * (S - 2) + [False]
    smp = eng.make_sampler("dpmpp2m", S, meta["cfg"], DEV, discretization="edm")
    smp.fused = False
    unf = eng.run_sampler(smp, x0, c, uc)
    close(fused, g["x_dpmpp2m_edm"], TOL_TRAJ, "dpmpp2m edm (fused)")
    close(unf, g["x_dpmpp2m_edm"], TOL_TRAJ, "dpmpp2m edm (unfused)")
    assert (eng.decode_first_stage(fused).cpu() - g["img_dpmpp2m_edm"]).abs().max().item() < 4e-3


def test_sdxl_img2img_and_pruned_base_stage(monkeypatch):
    """img2img_sdxl with DPM++ 2S ancestral on the EDM schedule (the face-fix re-entry, strength 0.3), and a Txt2Noisy-pruned base
    stage with HeunEDM on the EDM schedule, whose last step makes two UNet calls."""
    from cremage_amd import pipeline as P
    meta, g = load_golden("traj_sdxl_samplers_extra")
    eng = _tiny_engine(meta)
    B, L, seed = meta["B"], meta["L"], meta["seed"]
    c, uc = _cond("sxi2i", B, seed)
    img = synth_input("sxi2i.img", (B, 3, 2 * L, 2 * L), seed, 0.5).clamp(-1, 1).to(DEV)
    en, fn = synth_input("sxi2i.enc_noise", (B, 4, L, L), seed).to(DEV), synth_input("sxi2i.noise", (B, 4, L, L), seed).to(DEV)
    S, k = meta["i2i_steps"], meta["i2i_strength"]
    with recorded_noise(monkeypatch, "sxi2i", seed) as dr:
        images, x = P.img2img_sdxl(eng, img, c, uc, steps=S, strength=k, cfg_scale=meta["cfg"], enc_noise=en, fwd_noise=fn,
                                   sampler="DPMPP2SAncestral", discretization="edm")
    assert len(dr) == meta["draws"]["i2i"]
    close(x, g["x_i2i"], TOL_TRAJ, "img2img dpmpp2s edm")
    assert (images.cpu() - ((g["img_i2i"] + 1) / 2).clamp(0, 1)).abs().max().item() < 2e-3

    S, k = meta["t2n_steps"], meta["t2n_strength"]
    c, uc = _cond("sxt2n", B, seed)
    x0 = synth_input("sxt2n.x0", (B, 4, L, L), seed).to(DEV)
    n_steps = len(g["sigmas_t2n"]) - 1

    def unfused():
        smp = eng.make_sampler("heun_edm", S, meta["cfg"], DEV, stage2strength=k, discretization="edm")
        smp.fused = False
        return eng.run_sampler(smp, x0, c, uc)
    fused, unf, _, _ = _run_both(monkeypatch, eng, "sxt2n", seed,
                                 lambda: eng.sample(x0, c, uc, S, meta["cfg"], sampler="heun_edm", discretization="edm", stage2strength=k),
                                 unfused, _expected_kinds("heun_edm", n_steps, t2n=True))
    close(fused, g["x_t2n"], TOL_TRAJ, "pruned base heun edm (fused)")
    close(unf, g["x_t2n"], TOL_TRAJ, "pruned base heun edm (unfused)")


def _fused_vs_unfused(monkeypatch, key, opts, expect, tag):
    """6 steps of `key` on the legacy schedule with `opts` on the tiny engine: fused against unfused with the same recorded noise
    within 1e-5 relative, the fused launches `expect`; returns the two runs' draw counts."""
    meta, _ = load_golden(f"traj_sdxl_{key}")
    eng = _tiny_engine(meta)
    B, L, S, seed = meta["B"], meta["L"], meta["S"], meta["seed"]
    assert S == 6
    c, uc = _cond(tag, B, seed)
    x0 = synth_input(tag + ".x0", (B, 4, L, L), seed).to(DEV)

    def unfused():
        smp = eng.make_sampler(key, S, meta["cfg"], DEV, options=opts)
        smp.fused = False
        return eng.run_sampler(smp, x0, c, uc)
    fused, unf, nf, nu = _run_both(monkeypatch, eng, tag, seed, lambda: eng.sample(x0, c, uc, S, meta["cfg"], sampler=key, options=opts),
                                   unfused, expect(S))
    assert torch.isfinite(fused).all()
    r = rel_l2(fused.cpu(), unf.cpu())
    print(f"\n[{tag}] fused vs unfused rel-L2 {r:.3e}")
    assert r <= 1e-5
    return nf, nu, S


@pytest.mark.parametrize("order", [1, 2, 3])
def test_sdxl_lms_low_orders_fused(order, monkeypatch):
    """LinearMultistep below order 4: the fused executor's derivative ring has `order` slots."""
    _fused_vs_unfused(monkeypatch, "linear_multistep", {"sampler_order": order}, lambda S: [("lms", False)] * S, f"lms.order{order}")


def test_sdxl_euler_ancestral_eta_s_noise_fused(monkeypatch):
    """EulerAncestral with eta 0.5 and s_noise 1.1: the euler_a step with non-default scalars; one draw per step in both paths."""
    nf, nu, S = _fused_vs_unfused(monkeypatch, "euler_ancestral", {"sampler_eta": 0.5, "sampler_s_noise": 1.1},
                                  lambda S: _expected_kinds("euler_ancestral", S), "euler_a.eta05")
    assert nf == nu == S
