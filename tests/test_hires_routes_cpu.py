"""Hires fix and ControlNet img2img, the parts that need no GPU: the bilinear tables of crg_resize_noise against F.interpolate,
DDIMSampler.decode with the ControlNet dict conditioning, the composition of the new routes through their torch (unfused) paths
against fixtures made by the reference's own classes (tools/gen_golden_hires_routes.py), the error and default behaviour, and the
binding of the new entry point.  The networks are the CPU oracle's (oracle/ref_cpu.py) behind the interfaces the samplers use: the
HIP modules have no CPU path."""
import functools

import pytest
import torch
import torch.nn.functional as F

from cremage_amd.synth import synth_input
from oracle import ref_cpu as R
from tests.conftest import load_golden, max_abs, synth_state_dict

RESIZE_CASES = [((2, 4, 33, 47), 2.0), ((2, 4, 33, 47), 1.5), ((2, 4, 33, 47), 1.25), ((1, 4, 8, 8), 2.0)]


def table_blend(x, factor):
    """crg_resize_noise's gather and blend in torch: four values per output, horizontally then vertically."""
    from cremage_amd import ops
    h, w = x.shape[-2:]
    y0, y1, wy0, wy1 = ops.bilinear_tables(h, ops.upscaled_size(h, factor), factor)
    x0, x1, wx0, wx1 = ops.bilinear_tables(w, ops.upscaled_size(w, factor), factor)
    r0, r1 = x[:, :, y0], x[:, :, y1]
    top = wx0 * r0[..., x0] + wx1 * r0[..., x1]
    bot = wx0 * r1[..., x0] + wx1 * r1[..., x1]
    return wy0[:, None] * top + wy1[:, None] * bot


@pytest.mark.parametrize("shape,factor", RESIZE_CASES)
def test_bilinear_tables_match_interpolate(shape, factor):
    """ops.bilinear_tables + a torch gather-blend == F.interpolate(bilinear, align_corners=False) within 1e-6 of max|ref| (a wrong index
    formula misses by orders of magnitude, the two-rounding form of the source coordinate by 3x).  1.25 on 33 x 47 gives 41 x 58: the
    floor of the output size; every factor clamps the first source coordinate at 0, factor 2 also the last one at the last row."""
    from cremage_amd import ops
    x = synth_input(f"resize.x{factor}", shape, 11)
    ref = F.interpolate(x, scale_factor=factor, mode="bilinear", align_corners=False)
    got = table_blend(x, factor)
    assert got.shape == ref.shape
    if factor == 1.25:
        assert tuple(ref.shape[-2:]) == (41, 58)
    i0, i1, w0, w1 = ops.bilinear_tables(shape[2], ref.shape[2], factor)
    assert i0[0] == 0 and w1[0] == 0 and i1.max() == shape[2] - 1  # the lower clamp: the first source coordinate is negative
    if factor == 2.0:
        assert i0[-1] == i1[-1] == shape[2] - 1  # the upper clamp: the last source coordinate lies past the last row
    assert torch.equal(w0 + w1, torch.ones_like(w0))
    err = (got - ref).abs().max().item()
    print(f"\n[tables {shape} x{factor}] max abs {err:.3e}, bound {1e-6 * ref.abs().max().item():.3e}")
    assert err <= 1e-6 * ref.abs().max().item()


class _CpuControlLDM:
    """The oracle's ControlLDM.apply_model behind what the samplers and the pipeline ask of an LDM."""
    num_timesteps = 1000
    device = torch.device("cpu")

    def __init__(self, meta):
        from cremage_amd.cldm_hip import ControlledUnetModel, ControlNet
        from cremage_amd.samplers import make_alphas_cumprod
        cfg = meta["unet"]
        self.cfg = cfg
        self.cn_sd = synth_state_dict(ControlNet(hint_channels=3, **{k: v for k, v in cfg.items() if k != "out_channels"}), meta["seed"], "cn.")
        self.un_sd = synth_state_dict(ControlledUnetModel(**cfg), meta["seed"], "unet.")
        self.alphas_cumprod = make_alphas_cumprod(1000)
        self.calls = []

    def apply_model(self, x, t, cond, **kw):
        assert isinstance(cond, dict)
        self.calls.append(cond)
        return R.control_ldm_apply_model(self.un_sd, self.cn_sd, self.cfg, x, t.float(), cond["c_crossattn"], cond["c_concat"])


@functools.lru_cache(maxsize=None)
def _control_ldm():
    return _CpuControlLDM(load_golden("traj_cn_ddim_img2img")[0])


def test_ddim_decode_dict_conditioning_cpu():
    """DDIMSampler.decode with {"c_crossattn", "c_concat"} dicts under CFG (a TypeError before: torch.cat of two dicts) reproduces
    the reference's DDIMControlNetSampler on the CPU; bound: that of the CPU test of traj_ddim_img2img (tests/test_oracle_golden.py)."""
    from cremage_amd.samplers import DDIMSampler
    meta, g = load_golden("traj_cn_ddim_img2img")
    ldm = _control_ldm()
    B, seed = meta["B"], meta["seed"]
    c, uc = synth_input("cni2i.c", (B, 77, 96), seed), synth_input("cni2i.uc", (B, 77, 96), seed)
    hint = g["hint"]
    smp = DDIMSampler(ldm)
    smp.make_schedule(ddim_num_steps=meta["S"], ddim_eta=0.0)
    t_enc = meta["t_enc"]
    z_enc = smp.stochastic_encode(g["init_latent"], torch.tensor([t_enc] * B), noise=g["fwd_noise"])
    assert max_abs(z_enc, g["z_enc"]) < 1e-4
    del ldm.calls[:]
    keep = g["z_enc"].clone()
    x = smp.decode(g["z_enc"], {"c_crossattn": [c], "c_concat": [hint]}, t_enc, unconditional_guidance_scale=meta["cfg"],
                   unconditional_conditioning={"c_crossattn": [uc], "c_concat": [hint]})
    assert torch.equal(g["z_enc"], keep)
    assert len(ldm.calls) == t_enc and all(d is ldm.calls[0] for d in ldm.calls)  # one doubled conditioning for the whole decode
    assert ldm.calls[0]["c_concat"][0].shape[0] == 2 * B
    print(f"\n[cn ddim decode cpu] max abs {max_abs(x, g['x']):.3e}")
    assert max_abs(x, g["x"]) < 1e-3


def test_txt2img_hires_controlnet_latent_cpu(monkeypatch):
    """txt2img_hires(upscaler="latent", hint=, hint_hires=) on the CPU: both passes with dict conditioning, the second with the hires
    hint, through the torch pair (F.interpolate + stochastic_encode) - the unfused fallback of ops.upscale_noise."""
    from cremage_amd import ops
    from cremage_amd import pipeline as P
    meta, g = load_golden("traj_cn_hires_latent")
    ldm = _control_ldm()
    B, L, seed, f = meta["B"], meta["L"], meta["seed"], meta["factor"]
    c, uc = synth_input("cnhires.c", (B, 77, 96), seed), synth_input("cnhires.uc", (B, 77, 96), seed)
    monkeypatch.setattr(ops, "upscale_noise", lambda *a, **k: pytest.fail("the launch has no CPU path"))
    del ldm.calls[:]
    images, x, base = P.txt2img_hires(ldm, c, uc, steps=meta["S"], sampler=meta["sampler"], cfg_scale=meta["cfg"], height=8 * L,
                                      width=8 * L, factor=f, strength=meta["strength"], x0=g["x0"], fwd_noise=g["fwd_noise"],
                                      upscaler="latent", hint=g["hint"], hint_hires=g["hint_hires"], decode=False)
    assert images is None and tuple(x.shape) == (B, 4, f * L, f * L)
    hints = [tuple(d["c_concat"][0].shape[-2:]) for d in ldm.calls]
    assert hints == [(8 * L, 8 * L)] * meta["S"] + [(8 * L * f, 8 * L * f)] * meta["t_enc"]
    print(f"\n[cn hires latent cpu] base {max_abs(base, g['base']):.3e} latent {max_abs(x, g['x']):.3e}")
    assert max_abs(base, g["base"]) < 2e-3   # the CPU bounds of traj_hires_latent (tests/test_oracle_golden.py)
    assert max_abs(x, g["x"]) < 3e-3


class _CpuSgmUNet(torch.nn.Module):
    def __init__(self, meta):
        super().__init__()
        from cremage_amd.sgm_hip.unet import UNetModel
        self.cfg = meta["unet"]
        self.sd = synth_state_dict(UNetModel(**self.cfg), meta["seed"], "sgm_unet.")
        self.vectors = []

    def forward(self, x, timesteps=None, context=None, y=None, **kw):
        self.vectors.append(y)
        return R.sgm_unet_forward(self.sd, self.cfg, x, timesteps.float(), context, y)


def _sdxl_case():
    meta, g = load_golden("traj_sdxl_hires_latent")
    B, seed = meta["B"], meta["seed"]
    ctx_c, ctx_uc = synth_input("xlhires.c", (B, 77, 128), seed), synth_input("xlhires.uc", (B, 77, 128), seed)
    c, uc = {"crossattn": ctx_c, "vector": g["cv"]}, {"crossattn": ctx_uc, "vector": g["ucv"]}
    c2, uc2 = {"crossattn": ctx_c, "vector": g["cv2"]}, {"crossattn": ctx_uc, "vector": g["ucv2"]}
    return meta, g, c, uc, c2, uc2


def test_txt2img_sdxl_hires_latent_cpu():
    """txt2img_sdxl_hires(upscaler="latent") on the CPU, factor 1.5 (8 x 8 -> 12 x 12): base pass, img2img_latent's torch expression
    on the Img2Img-pruned schedule with the second pass' own conditioning; and c_hires=None reuses c."""
    from cremage_amd import pipeline as P
    from cremage_amd.sgm_hip.sampling import DiffusionEngine
    meta, g, c, uc, c2, uc2 = _sdxl_case()
    L = meta["L"]
    net = _CpuSgmUNet(meta)
    eng = DiffusionEngine(net, torch.nn.Identity(), meta["scale_factor"])
    kw = dict(steps=meta["S"], cfg_scale=meta["cfg"], height=8 * L, width=8 * L, factor=meta["factor"], strength=meta["strength"],
              upscaler="latent", x0=g["x0"], fwd_noise=g["fwd_noise"], decode=False)
    images, x, base = P.txt2img_sdxl_hires(eng, c, uc, c_hires=c2, uc_hires=uc2, **kw)
    assert images is None and tuple(x.shape) == tuple(g["x"].shape) == (meta["B"], 4, 12, 12)
    print(f"\n[sdxl hires latent cpu] base {max_abs(base, g['base']):.3e} latent {max_abs(x, g['x']):.3e}")
    assert max_abs(base, g["base"]) < 2e-3   # the CPU bounds of traj_sdxl_img2img (tests/test_oracle_golden.py)
    assert max_abs(x, g["x"]) < 2e-3
    second = net.vectors[meta["S"]:]
    assert second and all(torch.equal(v, torch.cat([uc2["vector"], c2["vector"]])) for v in second)
    # c_hires / uc_hires None: the second pass sees c / uc again
    del net.vectors[:]
    _, x_same, _ = P.txt2img_sdxl_hires(eng, c, uc, **kw)
    assert all(torch.equal(v, torch.cat([uc["vector"], c["vector"]])) for v in net.vectors) and len(net.vectors) > meta["S"]
    assert not torch.equal(x_same, x)


def test_unknown_upscaler_raises():
    from cremage_amd import pipeline as P
    meta, g, c, uc, _, _ = _sdxl_case()
    with pytest.raises(ValueError, match="latent.*lanczos"):
        P.txt2img_sdxl_hires(None, c, uc, upscaler="bicubic")
    with pytest.raises(ValueError, match="latent.*lanczos"):
        P.txt2img_hires(None, c["crossattn"], uc["crossattn"], upscaler="esrgan")
    assert P._upscaler("Latent") == "latent" and P._upscaler("Lanczos") == "lanczos"  # Cremage's menu spells them capitalised


def test_encode_scalars_equal_stochastic_encode():
    """The host scalars ops.upscale_noise gets are the coefficients stochastic_encode gathers, bit for bit."""
    from cremage_amd import pipeline as P
    smp = P.SAMPLERS["dpmpp_2m"](_control_ldm())
    x0, noise = synth_input("enc.x0", (2, 4, 5, 7), 3), synth_input("enc.noise", (2, 4, 5, 7), 3)
    for t_enc, steps in [(3, 6), (10, 20), (1, 7), (29, 30)]:
        a, s = smp.encode_scalars(t_enc, steps)
        ref = smp.stochastic_encode(x0, torch.tensor([t_enc] * 2), sampling_steps=steps, noise=noise)
        assert torch.equal(a * x0 + s * noise, ref), (t_enc, steps)


def test_resize_noise_is_bound():
    """crg_resize_noise is declared, bound, and exported by the bf16 and the fp16 library alike (it is fp32 in both)."""
    import ctypes
    import os
    from cremage_amd import _lib
    assert "crg_resize_noise" in _lib.SIGNATURES
    res, args = _lib.SIGNATURES["crg_resize_noise"]
    assert res is ctypes.c_int and len(args) == 17
    here = os.path.dirname(_lib.LIB_PATH)
    for name in ("libcrg_hip.so", "libcrg_hip_f16.so"):
        assert hasattr(ctypes.CDLL(os.path.join(here, name)), "crg_resize_noise"), name
    from cremage_amd import ops
    with pytest.raises(_lib.CrgError):
        ops.upscale_noise(torch.zeros(1, 4, 8, 8), 2.0)  # no CPU fallback
