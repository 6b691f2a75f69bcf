"""The rest of Cremage's SD1.5 sampler menu on a real MI355X: every kind and branch of crg_cfg_kstep against the CPU fp32 chain (with
the buffers a branch must not read filled with NaN), the nine 6-step tiny-LDM trajectories through the fused and the unfused executor,
hires-fix with DPM++ 2M and a ControlNet run with DPM++ SDE, against fixtures made by the reference's own k_diffusion functions and
Cremage's sampler classes (tools/gen_golden_sd15_samplers.py)."""
import functools

import pytest
import torch

from cremage_amd.synth import synth_input
from tests.conftest import load_golden, rel_l2
from tests.test_hip_models import DEV, TOL_TRAJ, close
from tests.test_sd15_samplers_cpu import Recorded, same_calls

pytestmark = pytest.mark.gpu

SHAPE, CFG = (2, 4, 33, 47), 7.5  # a ragged element count, more than one block
KEYS = ["heun", "dpm2", "dpm2_a", "lms", "dpmpp_2s_a", "dpmpp_sde", "dpmpp_2m", "dpmpp_2m_sde", "dpmpp_3m_sde"]
# latent bound per sampler: TOL_TRAJ, the bound of the Euler trajectories on the same tiny nets, precision and decoder - except DPM2 and
# DPM2 A, measured on an MI355X at rel-L2 1.432e-4 and 1.172e-4 (fused and unfused bit-identical, rel-L2 0: the step kernels are not
# the cause; the midpoint derivative times the full step amplifies the fp32-class UNet's own error): twice the measured value
TOL_KEY = {"dpm2": 2.9e-4, "dpm2_a": 2.4e-4}
MENU = {"heun": "Heun", "dpm2": "DPM2", "dpm2_a": "DPM2 A", "lms": "LMS", "dpmpp_2s_a": "DPM++ 2S A", "dpmpp_sde": "DPM++ SDE",
        "dpmpp_2m": "DPM++ 2M", "dpmpp_2m_sde": "DPM++ 2M SDE", "dpmpp_3m_sde": "DPM++ 3M SDE"}


def _den(eps2, xin, c_out, cfg):
    b = xin.shape[0]
    den_u = eps2[:b] * c_out + xin
    den_c = eps2[b:] * c_out + xin
    return den_u + cfg * (den_c - den_u)


def _t(name, scale=1.0):
    return synth_input("kstep." + name, SHAPE, 11) * scale


def _eps(name):
    return synth_input("kstep." + name, (2 * SHAPE[0],) + SHAPE[1:], 11)


def _check(got, ref, what):
    """within 1e-6 of max|ref| (the fp32 chain differs by the device's division and nothing else)"""
    assert torch.isfinite(got).all(), what
    assert (got.cpu() - ref).abs().max().item() <= 1e-6 * ref.abs().max().item(), what


def _dev(*ts):
    return [t.to(DEV).contiguous() for t in ts]


def _nan():
    return torch.full(SHAPE, float("nan"), device=DEV)


def _all_nan(*ts):
    return all(torch.isnan(t).all().item() for t in ts)


def test_kstep_dpm2_2():
    """d2 = (x2 - den(x2)) / sigma; x = x + d2 * dt [+ (z * s_noise) * sigma_up]: x2 read and left alone, noise read only with add_noise."""
    from cremage_amd import ops
    x, x2, z, eps2 = _t("x", 10.0), _t("x2", 8.0), _t("z"), _eps("e")
    sigma, c_out, dt, up, s_noise = 6.25, -6.25, -4.5, 2.5, 0.9
    den = _den(eps2, x2, c_out, CFG)
    base = x + ((x2 - den) / sigma) * dt
    for add in (True, False):
        xg, eg, x2g, zg = _dev(x, eps2, x2, z)
        spare, old = _nan(), [_nan(), _nan()]
        ops.cfg_kstep_("dpm2_2", xg, eg, c_out, CFG, sigma=sigma, dt=dt, x2=x2g, den_out=spare, old=old, noise=zg if add else _nan(),
                       sigma_up=up, s_noise=s_noise, add_noise=add)
        _check(xg, base + (z * s_noise) * up if add else base, f"dpm2_2 noise={add}")
        assert torch.equal(x2g.cpu(), x2) and _all_nan(spare, *old)


def test_kstep_sde_1():
    """x2 = m0 * x - m1 * den; x2 = x2 + (z * s_noise) * sigma_up: x is not written."""
    from cremage_amd import ops
    x, z, eps2 = _t("x", 10.0), _t("z"), _eps("e1")
    m, c_out, up, s_noise = (0.75, -0.4), -9.4, 1.5, 1.1
    base = m[0] * x - m[1] * _den(eps2, x, c_out, CFG)
    for add in (True, False):
        xg, eg, zg = _dev(x, eps2, z)
        x2g, spare, old = _nan(), _nan(), [_nan(), _nan()]
        ops.cfg_kstep_("sde_1", xg, eg, c_out, CFG, x2=x2g, den_out=spare, old=old, m=m, noise=zg if add else _nan(), sigma_up=up,
                       s_noise=s_noise, add_noise=add)
        _check(x2g, base + (z * s_noise) * up if add else base, f"sde_1 noise={add}")
        assert torch.equal(xg.cpu(), x) and _all_nan(spare, *old)


def test_kstep_sde_2m():
    """last; first step (no old) and later steps (have_old), with and without noise; den_out always receives den."""
    from cremage_amd import ops
    x, z, old, eps2 = _t("x", 10.0), _t("z"), _t("old", 3.0), _eps("e2")
    c_out, a, c1, c2, p, s_noise = -5.5, 0.3125, 0.6875, 0.41, (3.4, 0.93), 1.05
    den = _den(eps2, x, c_out, CFG)
    for last, have_old, add in ((True, True, True), (False, False, True), (False, False, False), (False, True, True), (False, True, False)):
        ref = den if last else a * x + c1 * den
        if not last and have_old:
            ref = ref + c2 * (den - old)
        if not last and add:
            ref = ref + ((z * p[0]) * p[1]) * s_noise
        reads_old, reads_z = have_old and not last, add and not last
        xg, eg, zg, og = _dev(x, eps2, z, old)
        dg, og2, unread_z, unread_old = _nan(), _nan(), _nan(), _nan()
        ops.cfg_kstep_("sde_2m", xg, eg, c_out, CFG, den_out=dg, old=[og if reads_old else unread_old, og2], x2=_nan(),
                       noise=zg if reads_z else unread_z, a=a, c1=c1, c2=c2, p=p, s_noise=s_noise, last=last, have_old=have_old, add_noise=add)
        what = f"sde_2m last={last} have_old={have_old} noise={add}"
        _check(xg, ref, what)
        _check(dg, den, what + " den_out")
        assert torch.equal(og.cpu(), old) and _all_nan(og2, unread_z, unread_old), what


def test_kstep_sde_3m():
    """last and the orders 1, 2, 3, with and without noise; old[] past what the order reads stays unread."""
    from cremage_amd import ops
    x, z, den1, den2, eps2 = _t("x", 10.0), _t("z"), _t("d1", 3.0), _t("d2", 3.0), _eps("e3")
    c_out, a, c1, p, s_noise = -5.5, 0.21, 0.79, (3.4, 0.97), 0.95
    r0, r1, phi2, phi3 = 0.8125, 0.71, 0.43, -0.36
    rsum = float(torch.tensor(r0) + torch.tensor(r1))
    den = _den(eps2, x, c_out, CFG)
    for last, order, add in ((True, 3, True), (False, 1, True), (False, 1, False), (False, 2, True), (False, 2, False), (False, 3, True),
                             (False, 3, False)):
        ref = den if last else a * x + c1 * den
        if not last and order == 2:
            ref = ref + phi2 * ((den - den1) / r0)
        if not last and order == 3:
            d1_0, d1_1 = (den - den1) / r0, (den1 - den2) / r1
            d1 = d1_0 + ((d1_0 - d1_1) * r0) / rsum
            d2 = (d1_0 - d1_1) / rsum
            ref = (ref + phi2 * d1) - phi3 * d2
        if not last and add:
            ref = ref + ((z * p[0]) * p[1]) * s_noise
        n_old = 0 if last else order - 1
        xg, eg, zg, o1, o2 = _dev(x, eps2, z, den1, den2)
        dg, unread = _nan(), [_nan(), _nan(), _nan()]
        old = [o1 if n_old >= 1 else unread[0], o2 if n_old >= 2 else unread[1]]
        ops.cfg_kstep_("sde_3m", xg, eg, c_out, CFG, den_out=dg, old=old, noise=zg if add and not last else unread[2], a=a, c1=c1, p=p,
                       r=(r0, r1), rsum=rsum, phi2=phi2, phi3=phi3, order=order, s_noise=s_noise, last=last, add_noise=add)
        what = f"sde_3m last={last} order={order} noise={add}"
        _check(xg, ref, what)
        _check(dg, den, what + " den_out")
        assert torch.equal(o1.cpu(), den1) and torch.equal(o2.cpu(), den2) and _all_nan(*unread), what


def test_kstep_rejects_bad_arguments():
    from cremage_amd import _lib as L
    from cremage_amd import ops
    x, eps2 = torch.zeros(SHAPE, device=DEV), torch.zeros((2 * SHAPE[0],) + SHAPE[1:], device=DEV)
    b = lambda: torch.zeros(SHAPE, device=DEV)  # noqa: E731
    for kw, msg in ((dict(kind="dpm2_2", sigma=0.0, x2=b()), "positive"), (dict(kind="dpm2_2", sigma=1.0), "x2"),
                    (dict(kind="dpm2_2", sigma=1.0, x2=x), "alias"), (dict(kind="dpm2_2", sigma=1.0, x2=b(), add_noise=True), "noise"),
                    (dict(kind="sde_1"), "x2"), (dict(kind="sde_2m"), "den_out"), (dict(kind="sde_2m", den_out=x), "alias"),
                    (dict(kind="sde_2m", den_out=b(), have_old=True), "old"), (dict(kind="sde_2m", den_out=b(), add_noise=True), "noise"),
                    (dict(kind="sde_3m", den_out=b(), order=4), "order"), (dict(kind="sde_3m", den_out=b(), order=0), "order"),
                    (dict(kind="sde_3m", den_out=b(), order=2, r=(1.0, 0.0)), "old"),
                    (dict(kind="sde_3m", den_out=b(), order=2, old=[b()], r=(0.0, 0.0)), "r0"),
                    (dict(kind="sde_3m", den_out=b(), order=3, old=[b(), b()], r=(1.0, 0.0), rsum=1.0), "r1"),
                    (dict(kind="euler_a"), "unknown kind"), (dict(kind="sde_1", x2=torch.zeros(SHAPE[1:], device=DEV)), "expected"),
                    (dict(kind="sde_1", x2=torch.zeros(SHAPE)), "HIP device")):
        with pytest.raises(L.CrgError, match=msg):
            ops.cfg_kstep_(kw.pop("kind"), x, eps2, -1.0, CFG, **kw)
    buf = b()
    with pytest.raises(L.CrgError, match="alias"):
        ops.cfg_kstep_("sde_2m", x, eps2, -1.0, CFG, den_out=buf, old=[buf], have_old=True)


@functools.lru_cache(maxsize=None)
def _tiny_ldm():
    """The tiny LDM of traj_euler on the device (fp32-class UNet and VAE), built once for the module's trajectories."""
    from cremage_amd import pipeline as P
    meta, _ = load_golden("traj_sd15_heun")
    return P.build_synthetic_ldm(meta["unet"], meta["dd"], DEV, unet_dtype=torch.float32, vae_dtype=torch.float32, seed=meta["seed"])


def _expected_launches(key, S):
    """The fused launch of each UNet evaluation of an S-step run that ends at sigma 0: (kind, flag) - one_call, `advanced` or `last`."""
    pair = lambda a, b, end: [(a, False), (b, False)] * (S - 1) + [end]  # noqa: E731
    return {"heun": pair("heun_1", "heun_2", ("heun_1", True)), "dpm2": pair("heun_1", "dpm2_2", ("heun_1", True)),
            "dpm2_a": pair("heun_1", "dpm2_2", ("heun_1", True)), "lms": [("lms", False)] * S,
            "dpmpp_2s_a": pair("dpmpp2s_1", "dpmpp2s_2", ("dpmpp2s_1", True)), "dpmpp_sde": pair("sde_1", "dpmpp2s_2", ("heun_1", True)),
            "dpmpp_2m": [("dpmpp2m", False)] + [("dpmpp2m", True)] * (S - 2) + [("dpmpp2m", False)],
            "dpmpp_2m_sde": [("sde_2m", False)] * (S - 1) + [("sde_2m", True)],
            "dpmpp_3m_sde": [("sde_3m", False)] * (S - 1) + [("sde_3m", True)]}[key]


def _count_launches(m, calls):
    from cremage_amd import ops
    step, kstep, two_m = ops.cfg_sampler_step_, ops.cfg_kstep_, ops.cfg_dpmpp2m_step_
    m.setattr(ops, "cfg_sampler_step_", lambda kind, *a, **k: calls.append((kind, bool(k.get("one_call")))) or step(kind, *a, **k))
    m.setattr(ops, "cfg_kstep_", lambda kind, *a, **k: calls.append((kind, bool(k.get("last")))) or kstep(kind, *a, **k))
    m.setattr(ops, "cfg_dpmpp2m_step_", lambda *a: calls.append(("dpmpp2m", bool(a[-1]))) or two_m(*a))


@pytest.mark.parametrize("key", KEYS)
def test_sd15_trajectory(key, monkeypatch):
    """6 steps + decode of each sampler vs the reference's stack with its recorded noise: fused (one input build and one step launch
    per UNet evaluation, through txt2img and the menu name) and unfused (the torch executor); the launch sequence, the noise calls'
    number (and arguments), and fused against unfused within 1e-5."""
    from cremage_amd import pipeline as P
    meta, g = load_golden(f"traj_sd15_{key}")
    ldm = _tiny_ldm()
    B, L, S, seed = meta["B"], meta["L"], meta["S"], meta["seed"]
    c, uc = synth_input("traj.c", (B, 77, 96), seed).to(DEV), synth_input("traj.uc", (B, 77, 96), seed).to(DEV)
    x0 = synth_input("traj.x0", (B, 4, L, L), seed).to(DEV)
    keep = x0.clone()
    rec_f, rec_u = (Recorded(f"sd15.{key}", (B, 4, L, L), seed, DEV) for _ in range(2))
    if meta["draws"]:  # the recorded draws are reproducible from their names
        assert torch.equal(synth_input(f"sd15.{key}.noise0", (B, 4, L, L), seed), g["noise"][0])
    calls = []
    with monkeypatch.context() as m:
        _count_launches(m, calls)
        images, fused = P.txt2img(ldm, c, uc, steps=S, sampler=MENU[key], cfg_scale=meta["cfg"], height=8 * L, width=8 * L, x0=x0,
                                  noise_sampler=rec_f)
        assert calls == _expected_launches(key, S), calls
        del calls[:]
        smp = P.SAMPLERS[key](ldm, fused=False)
        smp.noise_sampler = rec_u
        unf, _ = smp.sample(S=S, conditioning=c, batch_size=B, shape=[4, L, L], unconditional_guidance_scale=meta["cfg"],
                            unconditional_conditioning=uc, x0=x0)
        assert calls == []
    assert torch.equal(x0, keep)
    assert torch.equal(smp.sigmas_host, g["sigmas"])
    assert len(rec_f.calls) == len(rec_u.calls) == meta["draws"] == g["calls"].shape[0]
    # the arguments: what the plan says, for both executors; the schedule's own sigmas equal the fixture's bit for bit, while DPM++ SDE
    # passes exp(-(-log(sigma))) values, which the CPU test pins (their last bit is the host CPU's log and exp)
    draws = torch.tensor([e["draw"] for e in smp.plan(S) if e["draw"] is not None], dtype=torch.float32).reshape(-1, 2)
    for rec in (rec_f, rec_u):
        assert same_calls(rec.calls, draws), key
    assert key == "dpmpp_sde" or torch.equal(draws, g["calls"])
    ref_img = ((g["img"] + 1) / 2).clamp(0, 1)
    r_f, r_u, r_fu = rel_l2(fused.cpu(), g["x"]), rel_l2(unf.cpu(), g["x"]), rel_l2(fused.cpu(), unf.cpu())
    pix = (images.cpu() - ref_img).abs().max().item()
    print(f"\n[sd15 {key}] latent rel-L2 fused {r_f:.3e} unfused {r_u:.3e}, fused vs unfused {r_fu:.3e}, pixel L-inf {pix:.3e}")
    close(fused, g["x"], TOL_KEY.get(key, TOL_TRAJ), f"sd15 {key} latent (fused)")
    close(unf, g["x"], TOL_KEY.get(key, TOL_TRAJ), f"sd15 {key} latent (unfused)")
    assert r_fu <= 1e-5
    assert pix < 2e-3


def test_sd15_hires_dpmpp_2m():
    """Hires-fix with the latent upscaler through txt2img_hires(sampler="DPM++ 2M"): the Karras schedule, stochastic_encode and the
    last t_enc + 1 sigmas (`denoising_steps`), vs Cremage's Dpmpp2mSampler."""
    from cremage_amd import pipeline as P
    meta, g = load_golden("traj_sd15_hires_dpmpp_2m")
    ldm = _tiny_ldm()
    B, L, seed, f = meta["B"], meta["L"], meta["seed"], meta["factor"]
    c, uc = synth_input("hires.c", (B, 77, 96), seed).to(DEV), synth_input("hires.uc", (B, 77, 96), seed).to(DEV)
    x0 = synth_input("hires.x0", (B, 4, L, L), seed).to(DEV)
    noise = synth_input("hires.noise", (B, 4, f * L, f * L), seed).to(DEV)
    images, x, base = P.txt2img_hires(ldm, c, uc, steps=meta["S"], sampler="DPM++ 2M", cfg_scale=meta["cfg"], height=8 * L, width=8 * L,
                                      factor=f, strength=meta["strength"], x0=x0, fwd_noise=noise)
    close(base, g["base"], TOL_TRAJ, "sd15 hires dpmpp_2m base latent")
    close(x, g["x"], TOL_TRAJ, "sd15 hires dpmpp_2m latent")
    ref_img = ((g["img"] + 1) / 2).clamp(0, 1)
    assert (images.cpu() - ref_img).abs().max().item() < 3e-3


def test_sd15_controlnet_dpmpp_sde(monkeypatch):
    """Dict conditioning ({"c_crossattn", "c_concat"}) through the plan executors: a tiny ControlLDM with `hint=` and DPM++ SDE, fused
    against unfused within 1e-5 with the same recorded noise."""
    from cremage_amd import pipeline as P
    meta, _ = load_golden("traj_sd15_dpmpp_sde")
    ldm = P.build_synthetic_control_ldm(meta["unet"], meta["dd"], DEV, unet_dtype=torch.float32, vae_dtype=torch.float32, seed=meta["seed"])
    B, L, S, seed = meta["B"], 8, 3, meta["seed"]
    c, uc = synth_input("traj.c", (B, 77, 96), seed).to(DEV), synth_input("traj.uc", (B, 77, 96), seed).to(DEV)
    x0 = synth_input("cn15.x0", (B, 4, L, L), seed).to(DEV)
    hint = (synth_input("cn15.hint", (B, 3, 8 * L, 8 * L), seed, 0.5).clamp(-1, 1) * 0.5 + 0.5).to(DEV)
    out = []
    for fused in (None, False):
        calls = []
        with monkeypatch.context() as m:
            _count_launches(m, calls)
            m.setitem(P.SAMPLERS, "dpmpp_sde", functools.partial(P.SAMPLERS["dpmpp_sde"], fused=fused))
            _, x = P.txt2img(ldm, c, uc, steps=S, sampler="dpmpp_sde", cfg_scale=meta["cfg"], height=8 * L, width=8 * L, x0=x0, hint=hint,
                             noise_sampler=Recorded("cn15", (B, 4, L, L), seed, DEV), decode=False)
        assert calls == (_expected_launches("dpmpp_sde", S) if fused is None else [])
        out.append(x)
    assert torch.isfinite(out[0]).all() and rel_l2(out[0].cpu(), out[1].cpu()) <= 1e-5


@pytest.mark.parametrize("key", ["dpm2_a", "dpmpp_sde"])
def test_sd15_txt2img_default_noise_per_image(key, monkeypatch):
    """txt2img without a noise_sampler: the run's noise up front from the plan's draw count (DPM2 A) or a BrownianPairNoise (DPM++
    SDE), per image generator - image 1 of a batch of two draws what it draws alone, and every planned draw is served."""
    from cremage_amd import pipeline as P
    from cremage_amd import samplers as K
    meta, _ = load_golden(f"traj_sd15_{key}")
    ldm = _tiny_ldm()
    L, S, seed = 8, 4, meta["seed"]
    c, uc = synth_input("traj.c", (2, 77, 96), seed).to(DEV), synth_input("traj.uc", (2, 77, 96), seed).to(DEV)
    real, seen = K.run_plan, []

    def recording(model, x, plan, noise_sampler=None, fused=None):
        assert noise_sampler is not None
        draws = []
        seen.append((K.plan_draws(plan), draws))
        return real(model, x, plan, lambda s, sn: draws.append(noise_sampler(s, sn)) or draws[-1], fused)
    monkeypatch.setattr(K, "run_plan", recording)
    gens = lambda idx: [torch.Generator(device=DEV).manual_seed(100 + i) for i in idx]  # noqa: E731
    _, both = P.txt2img(ldm, c, uc, steps=S, sampler=key, cfg_scale=meta["cfg"], height=8 * L, width=8 * L, generators=gens([0, 1]), decode=False)
    _, one = P.txt2img(ldm, c[1:], uc[1:], steps=S, sampler=key, cfg_scale=meta["cfg"], height=8 * L, width=8 * L, generators=gens([1]),
                       decode=False)
    (n2, d2), (n1, d1) = seen
    assert n2 == n1 == len(d2) == len(d1) == {"dpm2_a": S - 1, "dpmpp_sde": 2 * (S - 1)}[key]
    for a, b in zip(d2, d1):
        assert a.shape == (2, 4, L, L) and torch.equal(a[1:], b)
    assert torch.isfinite(both).all() and torch.isfinite(one).all()
