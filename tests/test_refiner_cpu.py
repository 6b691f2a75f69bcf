"""SDXL refiner stage and DPM++ 2M sampling, the parts that need no GPU: the refiner YAML plug point and the refiner UNet's parameter
contract against the reference's, the sigma lists of both discretization wrappers (alone and composed as init_sampling composes
them), the DPM++ 2M multiplier tables, and the unfused DPM++ 2M loop under an analytic denoiser - all against fixtures made by the
reference's own code (tools/gen_golden_refiner.py)."""
import hashlib
import os

import numpy as np
import pytest
import torch
import yaml

from tests.conftest import load_golden

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _refiner_yaml():
    return yaml.safe_load(open(os.path.join(REPO, "cremage_amd", "configs", "sd_xl_refiner-hip.yaml")))["model"]["params"]


def test_refiner_yaml_instantiates_hip_classes():
    from cremage_amd.ldm_hip.latent_diffusion import instantiate_from_config
    from cremage_amd.ldm_hip.vae import AutoencoderKL
    from cremage_amd.sgm_hip.unet import UNetModel
    p = _refiner_yaml()
    assert p["network_config"]["target"] == "cremage_amd.sgm_hip.unet.UNetModel"
    assert p["first_stage_config"]["target"] == "cremage_amd.ldm_hip.vae.AutoencoderKL"
    assert p["denoiser_config"]["target"] == "sgm.modules.diffusionmodules.denoiser.DiscreteDenoiser"
    assert p["conditioner_config"]["target"] == "sgm.modules.GeneralConditioner"
    meta, _ = load_golden("sgm_refiner_unet_full")
    assert p["network_config"]["params"] == meta["yaml_network_params"]  # only the target lines differ from sd_xl_refiner.yaml
    u = dict(p["network_config"]["params"], model_channels=64, num_head_channels=32, context_dim=[96] * 4, adm_in_channels=96)  # shrink
    unet = instantiate_from_config({"target": p["network_config"]["target"], "params": u})
    assert isinstance(unet, UNetModel)
    assert len(unet.middle_block[1].transformer_blocks) == 4
    assert tuple(unet.label_emb[0][0].weight.shape) == (256, 96)
    v = p["first_stage_config"]["params"]
    vae = instantiate_from_config({"target": p["first_stage_config"]["target"], "params": dict(v, ddconfig=dict(v["ddconfig"], ch=32))})
    assert isinstance(vae, AutoencoderKL)


def test_pipeline_refiner_config_is_the_yaml_one():
    from cremage_amd.pipeline import SDXL_REFINER_UNET
    assert SDXL_REFINER_UNET == _refiner_yaml()["network_config"]["params"]


def test_refiner_unet_state_dict_matches_reference_contract():
    """1 220 keys with the reference refiner UNet's names and shapes, 2 259 526 660 parameters (recorded from the reference's sgm
    UNetModel at the sd_xl_refiner.yaml settings)."""
    from cremage_amd.pipeline import SDXL_REFINER_UNET
    from cremage_amd.sgm_hip.unet import UNetModel
    meta, _ = load_golden("sgm_refiner_unet_full")
    with torch.device("meta"):
        unet = UNetModel(**SDXL_REFINER_UNET)
    items = sorted(f"{k}:{tuple(v.shape)}" for k, v in unet.state_dict().items())
    assert len(items) == meta["n_keys"] == 1220
    assert sum(p.numel() for p in unet.parameters()) == meta["n_params"] == 2259526660
    assert hashlib.sha1("\n".join(items).encode()).hexdigest() == meta["keys_sha1"]


@pytest.mark.parametrize("name", ["sgm_refiner_unet_tiny", "sgm_refiner_unet_small"])
def test_small_refiner_unets_match_reference_contract(name):
    from cremage_amd.sgm_hip.unet import UNetModel
    meta, _ = load_golden(name)
    with torch.device("meta"):
        unet = UNetModel(**meta["cfg"])
    items = sorted(f"{k}:{tuple(v.shape)}" for k, v in unet.state_dict().items())
    assert hashlib.sha1("\n".join(items).encode()).hexdigest() == meta["keys_sha1"]
    assert sum(p.numel() for p in unet.parameters()) == meta["n_params"]


def _tag(steps, strength):
    return f"{steps}_{int(round(strength * 100)):03d}"


def test_discretization_wrappers_match_reference():
    """Img2Img, Txt2Noisy (with original_steps) and Txt2Noisy around Img2Img (init_sampling's order), every steps x strength."""
    from cremage_amd.sgm_hip.sampling import (Img2ImgDiscretizationWrapper, LegacyDDPMDiscretization, Txt2NoisyDiscretizationWrapper,
                                              wrap_discretization)
    meta, g = load_golden("sdxl_sampler_toy")
    for steps in meta["steps"]:
        assert torch.equal(LegacyDDPMDiscretization()(steps), g[f"plain_{steps}"])
        for k in meta["strengths"]:
            tag = _tag(steps, k)
            assert torch.equal(Txt2NoisyDiscretizationWrapper(LegacyDDPMDiscretization(), k, original_steps=steps)(steps), g["t2n_" + tag])
            assert torch.equal(Img2ImgDiscretizationWrapper(LegacyDDPMDiscretization(), k)(steps), g["i2i_" + tag])
            assert torch.equal(wrap_discretization(LegacyDDPMDiscretization(), steps, stage2strength=k)(steps), g["t2n_" + tag])
            comp = wrap_discretization(LegacyDDPMDiscretization(), steps, img2img_strength=meta["i2i_for_composed"], stage2strength=k)
            assert torch.equal(comp(steps), g["comp_" + tag])
    # the docstring example of the reference: 30 steps at refiner strength 0.15 drop the last three sigmas of the base stage and
    # leave the refiner the last three steps
    assert len(g["t2n_30_015"]) == 28 and g["t2n_30_015"][-1] > 0
    assert len(g["i2i_30_015"]) == 4 and g["i2i_30_015"][0] == g["t2n_30_015"][-1]


def test_dpmpp2m_multipliers_bit_exact():
    """m1..m4 of every step of every recorded schedule equal the reference's get_variables / get_mult on the CPU bit for bit."""
    from cremage_amd.sgm_hip.sampling import dpmpp2m_multipliers
    meta, g = load_golden("sdxl_sampler_toy")
    n = 0
    for key in g:
        if not key.startswith("m_"):
            continue
        sig, ref = g[key[2:]], g[key].numpy()
        got = dpmpp2m_multipliers(sig)
        assert len(got) == ref.shape[0] == max(len(sig) - 1, 0), key
        for i, (m1, m2, m3, m4, adv) in enumerate(got):
            row = np.array([m1, m2, np.nan if m3 is None else m3, np.nan if m4 is None else m4], dtype=np.float32)
            assert np.array_equal(row, ref[i], equal_nan=True), (key, i, row, ref[i])
            assert np.float32(m1) == m1 and np.float32(m2) == m2  # fp32 values
            assert adv == (i > 0 and float(sig[i + 1]) > 0)
        if len(got):
            last = got[-1]
            if float(sig[-1]) == 0.0:
                assert last[0] == 0.0 and last[1] == -1.0 and not last[4]  # x = den on the last step
        n += 1
    assert n == len(meta["steps"]) * (1 + 3 * len(meta["strengths"]))


def toy_denoiser(inp, sigma, c):
    """tools/gen_golden_refiner.py toy_denoiser, restated."""
    s = sigma.reshape(-1, 1, 1, 1)
    return inp / (1.0 + s ** 2) + c["vector"].reshape(-1, 4, 1, 1) * (s / (1.0 + s))


def test_dpmpp2m_toy_trajectories_match_reference():
    """The unfused DPM++ 2M loop on the CPU: txt2img, the pruned base stage and the refiner stage continuing from it."""
    from cremage_amd.sgm_hip.sampling import DPMPP2MSampler, VanillaCFG, wrap_discretization
    from cremage_amd.synth import synth_input
    meta, g = load_golden("sdxl_sampler_toy")
    B, L, cfg, seed = meta["B"], meta["L"], meta["cfg"], meta["seed"]
    c = {"vector": synth_input("toy.cv", (B, 4), seed)}
    uc = {"vector": synth_input("toy.ucv", (B, 4), seed)}
    x0 = synth_input("toy.x0", (B, 4, L, L), seed)
    assert torch.equal(x0, g["x0"])
    keep = x0.clone()
    s = DPMPP2MSampler(meta["txt2img_steps"], VanillaCFG(cfg), device="cpu")
    torch.testing.assert_close(s(toy_denoiser, x0, cond=c, uc=uc), g["traj_txt2img"], rtol=1e-6, atol=1e-6)
    assert torch.equal(x0, keep)  # the caller's tensor is not scaled in place
    S, k = meta["stage_steps"], meta["stage_strength"]
    s = DPMPP2MSampler(S, VanillaCFG(cfg), device="cpu")
    s.discretization = wrap_discretization(s.discretization, S, stage2strength=k)
    z = s(toy_denoiser, x0, cond=c, uc=uc)
    torch.testing.assert_close(z, g["traj_base"], rtol=1e-6, atol=1e-6)
    s = DPMPP2MSampler(S, VanillaCFG(cfg), device="cpu")
    s.discretization = wrap_discretization(s.discretization, S, img2img_strength=k)
    sig = s.discretization(S)
    torch.testing.assert_close(s(toy_denoiser, z / torch.sqrt(1.0 + sig[0] ** 2.0), cond=c, uc=uc), g["traj_refiner"], rtol=1e-6, atol=1e-6)


def test_unknown_sdxl_sampler_is_an_error():
    from cremage_amd.sgm_hip.sampling import DiffusionEngine
    eng = DiffusionEngine(torch.nn.Identity(), torch.nn.Identity())
    with pytest.raises(ValueError):
        eng.make_sampler("dpmpp_sde", 10, 5.0, "cpu")
