"""SDXL refiner stage and DPM++ 2M sampling on a real MI355X, against fixtures made by the reference's own modules
(tools/gen_golden_refiner.py): the refiner UNet (sd_xl_refiner.yaml) tiny / small / full size, the fused CFG + DPM++ 2M step
kernel against the CPU fp32 chain, the DPM++ 2M trajectory through the fused and the unfused path, and the two-stage run
through pipeline.txt2img_sdxl_refined.  Tolerances are the ones tests/test_hip_models.py applies to the SDXL base."""
import pytest
import torch

from cremage_amd.synth import synth_fill_, synth_input
from tests.conftest import load_golden
from tests.test_hip_models import BF, DEV, TOL_NET, TOL_SDXL_BF16, TOL_TRAJ, close, prep

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def refiner_weights():
    """The full refiner's name-keyed synthetic weights (fp32, CPU) - one fill shared by the small and the full-size case, whose
    configs and seeds are the same."""
    from cremage_amd.sgm_hip.unet import UNetModel
    meta, _ = load_golden("sgm_refiner_unet_small")
    with torch.device("meta"):
        m = UNetModel(**meta["cfg"])
    m = synth_fill_(m.to_empty(device="cpu"), meta["seed"], prefix=meta["prefix"])
    return m.state_dict()


def _refiner_on_device(cfg, sd, dtype):
    from cremage_amd.sgm_hip.unet import UNetModel
    with torch.device("meta"):
        m = UNetModel(**cfg)
    m = m.to_empty(device=DEV)
    m.load_state_dict(sd)
    return m.to(dtype).eval()


def _run_unet(m, name, meta, g):
    B, L = meta["B"], meta["L"]
    x = synth_input(name + ".x", (B, 4, L, L), meta["seed"]).to(DEV)
    ctx = synth_input(name + ".ctx", (B, meta["m"], meta["ctx_dim"]), meta["seed"]).to(DEV)
    y = synth_input(name + ".y", (B, meta["cfg"]["adm_in_channels"]), meta["seed"]).to(DEV)
    with torch.no_grad():
        return m(x, timesteps=g["t"].to(DEV), context=ctx, y=y)


@pytest.mark.parametrize("dtype", [torch.float32, BF])
@pytest.mark.parametrize("name", ["sgm_refiner_unet_tiny", "sgm_refiner_unet_small"])
def test_refiner_unet_small(dtype, name, request):
    """The refiner UNet (model_channels 384, four levels, depth-4 transformers on levels 1 and 2 and the middle, 1280-wide context,
    2560-wide label_emb) against the reference's sgm UNetModel: tiny at small widths, small = the full config at L = 32."""
    from cremage_amd.sgm_hip.unet import UNetModel
    meta, g = load_golden(name)
    if name == "sgm_refiner_unet_tiny":
        m = prep(UNetModel(**meta["cfg"]), meta, dtype)
    else:
        m = _refiner_on_device(meta["cfg"], request.getfixturevalue("refiner_weights"), dtype)
    close(_run_unet(m, name, meta, g), g["y"], TOL_SDXL_BF16 if dtype == BF else TOL_NET[dtype], f"{name} {dtype}")


def test_refiner_unet_full_bf16(refiner_weights):
    """Full-size refiner (2 259 526 660 parameters), B = 2, 128x128 latent (1024^2 image), refiner-range timesteps, bf16."""
    from cremage_amd.pipeline import SDXL_REFINER_UNET
    meta, g = load_golden("sgm_refiner_unet_full")
    m = _refiner_on_device(SDXL_REFINER_UNET, refiner_weights, BF)
    assert sum(p.numel() for p in m.parameters()) == meta["n_params"] == 2259526660
    out = _run_unet(m, "sgm_refiner_unet_full", meta, g)
    r = close(out, g["y"], TOL_SDXL_BF16, "sgm_refiner_unet_full")
    print(f"\n[parity] SDXL refiner UNet full bf16: rel-L2 {r:.3e}")


def _dpm_chain(x, eps2, old, c_out, cfg, m1, m2, m3, m4, advanced):
    """The reference's per-element chain in fp32 torch on the CPU (DiscreteDenoiser, VanillaCFG, DPMPP2MSampler.sampler_step)."""
    b = x.shape[0]
    den_u = eps2[:b] * c_out + x
    den_c = eps2[b:] * c_out + x
    den = den_u + cfg * (den_c - den_u)
    if advanced:
        return m1 * x - m2 * (m3 * den - m4 * old), den
    return m1 * x - m2 * den, den


def test_cfg_dpmpp2m_step_kernel():
    """crg_cfg_dpmpp2m_step against the CPU fp32 chain on the first, a middle and the last step of a 30-step schedule (a ragged
    element count), and a standard step with an all-NaN old_den, which must not be read."""
    from cremage_amd import ops
    from cremage_amd.sgm_hip.sampling import LegacyDDPMDiscretization, dpmpp2m_multipliers
    sh = LegacyDDPMDiscretization()(30)
    mults = dpmpp2m_multipliers(sh)
    shape, cfg = (2, 4, 33, 47), 5.0
    for i in (0, 14, len(mults) - 1):
        m1, m2, m3, m4, adv = mults[i]
        assert adv == (0 < i < len(mults) - 1)
        x = synth_input(f"dpmk.x{i}", shape, 7) * float(sh[i])
        eps2 = synth_input(f"dpmk.e{i}", (2 * shape[0],) + shape[1:], 7)
        old = synth_input(f"dpmk.o{i}", shape, 7)
        c_out = -float(sh[i])
        ref, den = _dpm_chain(x, eps2, old, c_out, cfg, m1, m2, m3, m4, adv)
        xg, og = x.to(DEV).contiguous(), old.to(DEV).contiguous()
        ops.cfg_dpmpp2m_step_(xg, eps2.to(DEV).contiguous(), og, c_out, cfg, m1, m2, m3 or 0.0, m4 or 0.0, adv)
        assert (xg.cpu() - ref).abs().max().item() <= 1e-6 * ref.abs().max().item(), i
        assert (og.cpu() - den).abs().max().item() <= 1e-6 * den.abs().max().item(), i
    # a standard step never reads old_den: NaN there must not reach x
    m1, m2, _, _, adv = mults[0]
    x = synth_input("dpmk.nan.x", shape, 7)
    eps2 = synth_input("dpmk.nan.e", (2 * shape[0],) + shape[1:], 7)
    ref, den = _dpm_chain(x, eps2, None, -float(sh[0]), cfg, m1, m2, None, None, False)
    xg, og = x.to(DEV).contiguous(), torch.full(shape, float("nan"), device=DEV)
    ops.cfg_dpmpp2m_step_(xg, eps2.to(DEV).contiguous(), og, -float(sh[0]), cfg, m1, m2, 2.0, 1.0, False)
    assert torch.isfinite(xg).all() and torch.isfinite(og).all()
    assert (xg.cpu() - ref).abs().max().item() <= 1e-6 * ref.abs().max().item()


def _tiny_engine(meta):
    from cremage_amd.ldm_hip.vae import AutoencoderKL
    from cremage_amd.sgm_hip.sampling import DiffusionEngine
    from cremage_amd.sgm_hip.unet import UNetModel
    unet = synth_fill_(UNetModel(**meta["unet"]), meta["seed"], prefix="sgm_unet.")
    vae = synth_fill_(AutoencoderKL(meta["dd"], None, 4), meta["seed"], prefix="vae.")
    return DiffusionEngine(unet, vae, meta["scale_factor"]).to(DEV).eval()


def _cond(tag, B, cdim, vdim, seed):
    return ({"crossattn": synth_input(tag + ".c", (B, 77, cdim), seed).to(DEV), "vector": synth_input(tag + ".cv", (B, vdim), seed).to(DEV)},
            {"crossattn": synth_input(tag + ".uc", (B, 77, cdim), seed).to(DEV), "vector": synth_input(tag + ".ucv", (B, vdim), seed).to(DEV)})


def test_sdxl_trajectory_dpmpp2m_fused_and_unfused(monkeypatch):
    """6 DPM++ 2M steps + decode vs the reference's stack, through the fused path (one crg_cfg_dpmpp2m_step per step) and the unfused
    torch path; the two agree within 1e-5 relative."""
    from cremage_amd import ops
    from cremage_amd.sgm_hip.sampling import DPMPP2MSampler, VanillaCFG
    from tests.conftest import rel_l2
    meta, g = load_golden("traj_sdxl_dpmpp2m")
    eng = _tiny_engine(meta)
    B, L, S = meta["B"], meta["L"], meta["S"]
    c, uc = _cond("dpm2m", B, 128, 96, meta["seed"])
    x0 = synth_input("dpm2m.x0", (B, 4, L, L), meta["seed"]).to(DEV)
    keep = x0.clone()
    calls = []
    real = ops.cfg_dpmpp2m_step_
    monkeypatch.setattr(ops, "cfg_dpmpp2m_step_", lambda *a: calls.append(a[-1]) or real(*a))
    fused = eng.sample(x0, c, uc, S, meta["cfg"], sampler="dpmpp2m")
    assert calls == [False] + [True] * (S - 2) + [False]
    assert torch.equal(x0, keep)
    unfused = eng.run_sampler(DPMPP2MSampler(S, VanillaCFG(meta["cfg"]), device=x0.device, fused=False), x0, c, uc)
    assert len(calls) == S
    close(fused, g["x"], TOL_TRAJ, "sdxl dpmpp2m latent (fused)")
    close(unfused, g["x"], TOL_TRAJ, "sdxl dpmpp2m latent (unfused)")
    assert rel_l2(fused.cpu(), unfused.cpu()) <= 1e-5
    img = eng.decode_first_stage(fused)
    assert (img.cpu() - g["img"]).abs().max().item() < 4e-3


def test_sdxl_refined_two_stage_trajectory():
    """txt2img_sdxl_refined on a tiny base + tiny refiner (DPM++ 2M, 10 steps, strength 0.3) vs the reference's two-stage run: the
    pruned base stage's latents, the refiner's latents and the decoded image; refiner_strength 0 is txt2img_sdxl."""
    from cremage_amd import pipeline as P
    from cremage_amd.sgm_hip.sampling import LegacyDDPMDiscretization, wrap_discretization
    meta, g = load_golden("traj_sdxl_refiner")
    B, L, S, k, seed = meta["B"], meta["L"], meta["S"], meta["strength"], meta["seed"]
    # (bit-exact on the CPU that wrote the fixtures, tests/test_refiner_cpu.py; another host CPU may round the fp32 sqrt of the
    # schedule differently in the last place)
    torch.testing.assert_close(wrap_discretization(LegacyDDPMDiscretization(), S, stage2strength=k)(S), g["sigmas_base"], rtol=1e-6, atol=0)
    torch.testing.assert_close(wrap_discretization(LegacyDDPMDiscretization(), S, img2img_strength=k)(S), g["sigmas_refiner"], rtol=1e-6,
                               atol=0)
    base = P.build_synthetic_sdxl(meta["unet"], meta["dd"], DEV, unet_dtype=torch.float32, vae_dtype=torch.float32, seed=seed)
    refiner = P.build_synthetic_sdxl_refiner(meta["refiner_unet"], device=DEV, unet_dtype=torch.float32, seed=meta["refiner_seed"],
                                             first_stage=base.first_stage_model)
    assert refiner.first_stage_model is base.first_stage_model
    c, uc = _cond("refb", B, 128, 96, seed)
    c2, uc2 = _cond("refr", B, 96, 96, seed)
    x0 = synth_input("refb.x0", (B, 4, L, L), seed).to(DEV)
    images, z, x = P.txt2img_sdxl_refined(base, refiner, c, uc, c2, uc2, steps=S, refiner_strength=k, cfg_scale=meta["cfg"], height=2 * L,
                                          width=2 * L, x0=x0)
    close(z, g["z"], TOL_TRAJ, "refined: base-stage latent")
    close(x, g["x"], TOL_TRAJ, "refined: refiner latent")
    ref = ((g["img"] + 1) / 2).clamp(0, 1)
    assert images.shape == ref.shape and (images.cpu() - ref).abs().max().item() < 2e-3
    off, z0, x0_out = P.txt2img_sdxl_refined(base, refiner, c, uc, c2, uc2, steps=S, refiner_strength=0, cfg_scale=meta["cfg"],
                                             height=2 * L, width=2 * L, x0=x0)
    plain, xp = P.txt2img_sdxl(base, c, uc, steps=S, cfg_scale=meta["cfg"], height=2 * L, width=2 * L, x0=x0, sampler="dpmpp2m")
    assert torch.equal(x0_out, xp) and torch.equal(z0, xp) and torch.equal(off, plain)
