"""Hires fix and ControlNet img2img on a real MI355X: crg_resize_noise against the CPU fp32 chain, DDIMSampler.decode's fused executor
for dict conditioning, the latent hires routes of SD1.5 (ControlNet, DPM++ 2M) and SDXL (Euler EDM, factor 1.5) against fixtures made
by the reference's own classes (tools/gen_golden_hires_routes.py), and the "lanczos" routes against the composition of the package's
own public calls."""
import functools

import pytest
import torch
import torch.nn.functional as F

from cremage_amd.synth import synth_input
from tests.conftest import load_golden, rel_l2
from tests.test_hip_models import DEV, TOL_TRAJ, close
from tests.test_hires_routes_cpu import RESIZE_CASES, _sdxl_case

pytestmark = pytest.mark.gpu

# (a, s, d, with noise): DDIM / k-diffusion stochastic_encode, the plain upscale, SDXL do_img2img (d = sqrt(1 + s^2) != 1)
FORMS = [(0.8313, 0.5558, 1.0, True), (1.0, 0.0, 1.0, False), (1.0, 3.2, (1.0 + 3.2 ** 2) ** 0.5, True), (0.7, 0.0, 1.3, False)]
# 8x first stage (three down levels) for the pixel-space routes: pipeline sizes the latents as height // 8
DD8 = dict(double_z=True, z_channels=4, resolution=64, in_channels=3, out_ch=3, ch=32, ch_mult=[1, 1, 2, 2], num_res_blocks=1,
           attn_resolutions=[], dropout=0.0)


# ControlNet hires-fix latents: measured on an MI355X at rel-L2 1.097e-4 (first pass) and 1.056e-4 (second pass), above TOL_TRAJ (1e-4,
# the bound of the trajectories without a ControlNet).  The first pass runs no code of the hires route - it is txt2img(hint=) with
# DPM++ 2M - and two fp32-class networks (ControlNet and UNet) instead of one feed every step; as for DPM2 in
# tests/test_sd15_samplers_gpu.py the bound of such a case is twice its measured value.
TOL_CN_HIRES = {"base": 2.2e-4, "latent": 2.12e-4}


def _check(got, ref, what):
    """within 1e-6 of max|ref| (tests/test_sd15_samplers_gpu.py _check: the fp32 chain differs by the device's division, here also by
    ATen's contracted blend, and nothing else)"""
    assert torch.isfinite(got).all(), what
    err, bound = (got.cpu() - ref).abs().max().item(), 1e-6 * ref.abs().max().item()
    print(f"\n[{what}] max abs {err:.3e}, bound {bound:.3e}")
    assert err <= bound, what


@pytest.mark.parametrize("shape,factor", RESIZE_CASES)
def test_upscale_noise_matches_cpu_chain(shape, factor):
    """ops.upscale_noise vs (a * F.interpolate(x) + s * noise) / d on the CPU: ragged element counts over more than one block, the
    floor of the output size (1.25), every scalar form, noise present and None; the output starts as NaN and the inputs stay intact."""
    from cremage_amd import ops
    x = synth_input(f"resize.x{factor}", shape, 11)
    up = F.interpolate(x, scale_factor=factor, mode="bilinear", align_corners=False)
    noise = synth_input(f"resize.noise{factor}", tuple(up.shape), 11)
    xd, nd = x.to(DEV), noise.to(DEV)
    for a, s, d, noisy in FORMS:
        out = torch.full(tuple(up.shape), float("nan"), device=DEV)
        got = ops.upscale_noise(xd, factor, nd if noisy else None, a, s, d, out=out)
        assert got is out
        ref = (a * up + s * noise) / d if noisy else (a * up) / d
        _check(got, ref, f"upscale_noise {shape} x{factor} a={a} s={s} d={d:.4f} noise={noisy}")
        assert torch.equal(xd.cpu(), x) and torch.equal(nd.cpu(), noise)
    fresh = ops.upscale_noise(xd, factor)
    _check(fresh, up, f"upscale_noise {shape} x{factor} defaults")


def test_upscale_noise_past_2_31_elements():
    """32769 planes of 128 x 128 -> 256 x 256: 2^31 + 65536 outputs, so the last plane's flat indices do not fit 32 bits."""
    from cremage_amd import ops
    planes = 32769
    x = torch.zeros((1, planes, 128, 128), device=DEV)
    first, last = synth_input("resize.big0", (1, 1, 128, 128), 11), synth_input("resize.big1", (1, 1, 128, 128), 11)
    x[:, :1], x[:, -1:] = first.to(DEV), last.to(DEV)
    out = ops.upscale_noise(x, 2.0, None, 0.5, 0.0, 1.0)
    assert out.numel() > 2 ** 31
    for got, src, what in ((out[:, :1], first, "first plane"), (out[:, -1:], last, "last plane")):
        _check(got, 0.5 * F.interpolate(src, scale_factor=2.0, mode="bilinear", align_corners=False), "upscale_noise 2^31 " + what)
    assert not out[:, 1:-1].any()


def test_upscale_noise_rejects_bad_arguments():
    from cremage_amd import _lib as L
    from cremage_amd import ops
    x = torch.zeros((1, 4, 8, 8), device=DEV)
    for kw, msg in ((dict(noise=torch.zeros((1, 4, 8, 8), device=DEV)), "noise of shape"), (dict(d=0.0), "must not be 0"),
                    (dict(out=torch.zeros((1, 4, 16, 15), device=DEV)), "out of shape"), (dict(noise=torch.zeros(1, 4, 16, 16)), "HIP device")):
        with pytest.raises(L.CrgError, match=msg):
            ops.upscale_noise(x, 2.0, **kw)
    with pytest.raises(L.CrgError, match="NCHW"):
        ops.upscale_noise(x.to(torch.bfloat16), 2.0)


@functools.lru_cache(maxsize=None)
def _control_ldm(dd8=False):
    """The tiny ControlLDM of the fixtures on the device (fp32-class nets); `dd8`: with the 8x first stage instead of the fixtures' 2x."""
    from cremage_amd import pipeline as P
    meta, _ = load_golden("traj_cn_ddim_img2img")
    return P.build_synthetic_control_ldm(meta["unet"], DD8 if dd8 else meta["dd"], DEV, unet_dtype=torch.float32, vae_dtype=torch.float32,
                                         seed=meta["seed"])


def test_controlnet_img2img_fused_decode(monkeypatch):
    """pipeline.img2img(hint=): DDIMSampler.decode's fused executor (one crg_cfg_ddim_step per step, no elementwise chain) vs the
    reference's DDIMControlNetSampler; then decode on the same inputs with a callback, which forces the chain."""
    from cremage_amd import ops
    from cremage_amd import pipeline as P
    from cremage_amd.samplers import DDIMSampler
    meta, g = load_golden("traj_cn_ddim_img2img")
    ldm = _control_ldm()
    B, seed, t_enc = meta["B"], meta["seed"], meta["t_enc"]
    c, uc = synth_input("cni2i.c", (B, 77, 96), seed).to(DEV), synth_input("cni2i.uc", (B, 77, 96), seed).to(DEV)
    hint = g["hint"].to(DEV)
    steps, real = [], ops.cfg_ddim_step_
    with monkeypatch.context() as m:
        m.setattr(ops, "cfg_ddim_step_", lambda *a: steps.append(a[4:]) or real(*a))
        m.setattr(DDIMSampler, "p_sample_ddim", lambda *a, **k: pytest.fail("the chain ran"))
        images, x = P.img2img(ldm, g["img_in"].to(DEV), c, uc, steps=meta["S"], strength=meta["strength"], cfg_scale=meta["cfg"],
                              enc_noise=g["enc_noise"].to(DEV), fwd_noise=g["fwd_noise"].to(DEV), hint=hint)
    assert len(steps) == t_enc and all(sc[4] == 0.0 for sc in steps)
    close(x, g["x"], TOL_TRAJ, "cn ddim img2img latent (fused)")
    ref_img = ((g["img"] + 1) / 2).clamp(0, 1)
    assert (images.cpu() - ref_img).abs().max().item() < 2e-3
    # the chain: the same decode with a callback
    smp = DDIMSampler(ldm)
    smp.make_schedule(ddim_num_steps=meta["S"], ddim_eta=0.0)
    z_enc, seen = g["z_enc"].to(DEV), []
    cond, ucond = P._control_cond(c, uc, hint)
    kw = dict(unconditional_guidance_scale=meta["cfg"], unconditional_conditioning=ucond)
    chain = smp.decode(z_enc, cond, t_enc, callback=seen.append, **kw)
    fused = smp.decode(z_enc, cond, t_enc, **kw)
    assert seen == list(range(t_enc)) and torch.equal(z_enc.cpu(), g["z_enc"])
    r = rel_l2(fused.cpu(), chain.cpu())
    print(f"\n[cn ddim decode] fused vs chain rel-L2 {r:.3e}")
    close(chain, g["x"], TOL_TRAJ, "cn ddim img2img latent (chain)")
    close(fused, g["x"], TOL_TRAJ, "cn ddim img2img latent (fused, from the fixture's z_enc)")
    assert r <= TOL_TRAJ


def _count_upscales(m, calls):
    from cremage_amd import ops
    real = ops.upscale_noise
    m.setattr(ops, "upscale_noise", lambda *a, **k: calls.append(tuple(float(v) for v in a[3:6])) or real(*a, **k))
    m.setattr(F, "interpolate", lambda *a, **k: pytest.fail("the torch pair ran"))


def test_txt2img_hires_controlnet_latent(monkeypatch):
    """txt2img_hires(upscaler="latent", hint=, hint_hires=) with DPM++ 2M, 8 x 8 -> 16 x 16: one ops.upscale_noise launch between the
    passes (a, s of stochastic_encode, d = 1), the second pass with the hires hint - which the ControlNet's one-entry hint cache then
    holds."""
    from cremage_amd import pipeline as P
    meta, g = load_golden("traj_cn_hires_latent")
    ldm = _control_ldm()
    B, L, seed, f = meta["B"], meta["L"], meta["seed"], meta["factor"]
    c, uc = synth_input("cnhires.c", (B, 77, 96), seed).to(DEV), synth_input("cnhires.uc", (B, 77, 96), seed).to(DEV)
    calls = []
    with monkeypatch.context() as m:
        _count_upscales(m, calls)
        images, x, base = P.txt2img_hires(ldm, c, uc, steps=meta["S"], sampler=meta["sampler"], cfg_scale=meta["cfg"], height=8 * L,
                                          width=8 * L, factor=f, strength=meta["strength"], x0=g["x0"].to(DEV),
                                          fwd_noise=g["fwd_noise"].to(DEV), hint=g["hint"].to(DEV), hint_hires=g["hint_hires"].to(DEV))
    assert len(calls) == 1 and calls[0][2] == 1.0 and abs(calls[0][0] ** 2 + calls[0][1] ** 2 - 1.0) < 1e-6
    cached = ldm.control_model._hint_cache[0][0]
    assert tuple(cached.shape) == (2 * B, 3, 8 * L * f, 8 * L * f) and torch.equal(cached[B:].cpu(), g["hint_hires"])
    # the first pass again through the torch executor: what the fused step kernels add to the distance from the fixture
    smp = P.SAMPLERS["dpmpp_2m"](ldm, fused=False)
    unf, _ = smp.sample(S=meta["S"], conditioning=P._control_cond(c, uc, g["hint"].to(DEV))[0], batch_size=B, shape=[4, L, L],
                        unconditional_guidance_scale=meta["cfg"], unconditional_conditioning=P._control_cond(c, uc, g["hint"].to(DEV))[1],
                        x0=g["x0"].to(DEV))
    print(f"\n[cn hires latent] base rel-L2 {rel_l2(base.cpu(), g['base']):.3e} (torch executor {rel_l2(unf.cpu(), g['base']):.3e}, fused "
          f"vs torch {rel_l2(base.cpu(), unf.cpu()):.3e}) latent {rel_l2(x.cpu(), g['x']):.3e}")
    close(base, g["base"], TOL_CN_HIRES["base"], "cn hires base latent")
    close(x, g["x"], TOL_CN_HIRES["latent"], "cn hires latent")
    ref_img = ((g["img"] + 1) / 2).clamp(0, 1)
    assert (images.cpu() - ref_img).abs().max().item() < 3e-3


@functools.lru_cache(maxsize=None)
def _sdxl_engine(dd8=False):
    from cremage_amd import pipeline as P
    meta, _ = load_golden("traj_sdxl_hires_latent")
    return P.build_synthetic_sdxl(meta["unet"], DD8 if dd8 else meta["dd"], DEV, unet_dtype=torch.float32, vae_dtype=torch.float32,
                                  seed=meta["seed"])


def _to_dev(d):
    return {k: v.to(DEV) for k, v in d.items()}


def test_txt2img_sdxl_hires_latent(monkeypatch):
    """txt2img_sdxl_hires(upscaler="latent"), Euler EDM, factor 1.5 (8 x 8 -> 12 x 12): one launch with a = 1, s = sigma_0 and
    d = sqrt(1 + sigma_0^2) of the Img2Img-pruned schedule, the second pass with its own conditioning."""
    from cremage_amd import pipeline as P
    meta, g, c, uc, c2, uc2 = _sdxl_case()
    eng, L = _sdxl_engine(), meta["L"]
    calls = []
    with monkeypatch.context() as m:
        _count_upscales(m, calls)
        images, x, base = P.txt2img_sdxl_hires(eng, _to_dev(c), _to_dev(uc), steps=meta["S"], cfg_scale=meta["cfg"], height=8 * L,
                                               width=8 * L, factor=meta["factor"], strength=meta["strength"], upscaler="latent",
                                               c_hires=_to_dev(c2), uc_hires=_to_dev(uc2), x0=g["x0"].to(DEV),
                                               fwd_noise=g["fwd_noise"].to(DEV))
    s0 = g["sigmas"][0]
    assert len(calls) == 1 and calls[0][0] == 1.0
    assert abs(calls[0][1] - float(s0)) <= 1e-6 * float(s0) and abs(calls[0][2] - float(torch.sqrt(1.0 + s0 ** 2.0))) <= 1e-6 * float(s0)
    print(f"\n[sdxl hires latent] base rel-L2 {rel_l2(base.cpu(), g['base']):.3e} latent {rel_l2(x.cpu(), g['x']):.3e}")
    close(base, g["base"], TOL_TRAJ, "sdxl hires base latent")
    close(x, g["x"], TOL_TRAJ, "sdxl hires latent")
    ref_img = ((g["img"] + 1) / 2).clamp(0, 1)
    assert (images.cpu() - ref_img).abs().max().item() < 3e-3


def test_txt2img_hires_lanczos_is_the_composition():
    """upscaler="lanczos" with a ControlNet hint == decode_images -> upscale_uint8 -> encode -> stochastic_encode -> the second pass,
    composed from the package's public calls with the same noises, bit for bit; sizes are `factor` times the first pass'.  (The
    second pass is the k-diffusion sampler's, as in the reference, not pipeline.img2img's DDIM.)"""
    from cremage_amd import pipeline as P
    from cremage_amd import postprocess as PP
    meta, _ = load_golden("traj_cn_hires_latent")
    ldm = _control_ldm(dd8=True)
    B, L, S, seed, f, cfg = meta["B"], meta["L"], meta["S"], meta["seed"], 2, meta["cfg"]
    c, uc = synth_input("cnhires.c", (B, 77, 96), seed).to(DEV), synth_input("cnhires.uc", (B, 77, 96), seed).to(DEV)
    x0 = synth_input("cnhires.x0", (B, 4, L, L), seed).to(DEV)
    hint = (synth_input("lz.hint", (B, 3, 8 * L, 8 * L), seed, 0.5).clamp(-1, 1) * 0.5 + 0.5).to(DEV)
    enc_noise, fwd_noise = (synth_input(n, (B, 4, f * L, f * L), seed).to(DEV) for n in ("lz.encnoise", "lz.fwdnoise"))
    kw = dict(steps=S, sampler="DPM++ 2M", cfg_scale=cfg, height=8 * L, width=8 * L, x0=x0)
    images, x, base = P.txt2img_hires(ldm, c, uc, factor=f, strength=0.5, fwd_noise=fwd_noise, enc_noise=enc_noise, upscaler="lanczos",
                                      hint=hint, **kw)
    assert tuple(base.shape) == (B, 4, L, L) and tuple(x.shape) == (B, 4, f * L, f * L) and tuple(images.shape) == (B, 3, 8 * L * f, 8 * L * f)
    # the composition
    first, base2 = P.txt2img(ldm, c, uc, hint=hint, **kw)
    assert torch.equal(base2, base) and tuple(first.shape) == (B, 3, 8 * L, 8 * L)
    scaled = PP.upscale_uint8(P.decode_images(ldm, base2), 8 * L * f, 8 * L * f).contiguous() * 2.0 - 1.0
    init = ldm.get_first_stage_encoding(ldm.encode_first_stage(scaled), enc_noise)
    smp = P.SAMPLERS["dpmpp_2m"](ldm)
    t_enc = int(0.5 * S)
    z_enc = smp.stochastic_encode(init, torch.tensor([t_enc] * B, device=DEV), sampling_steps=S, noise=fwd_noise)
    cond, ucond = P._control_cond(c, uc, PP.upscale_uint8(hint, 8 * L * f, 8 * L * f).contiguous())
    x2, _ = smp.sample(S=S, conditioning=cond, batch_size=B, shape=[4, f * L, f * L], unconditional_guidance_scale=cfg,
                       unconditional_conditioning=ucond, x0=z_enc, denoising_steps=t_enc)
    assert torch.isfinite(x).all() and torch.equal(x2, x)
    assert torch.equal(P.decode_images(ldm, x2), images)


def test_txt2img_sdxl_hires_lanczos_is_the_composition():
    """SDXL upscaler="lanczos" == txt2img_sdxl -> upscale_uint8 -> img2img_sdxl with the same noises, bit for bit, at factor 1.5."""
    from cremage_amd import pipeline as P
    from cremage_amd import postprocess as PP
    meta, g, c, uc, c2, uc2 = _sdxl_case()
    c, uc, c2, uc2 = (_to_dev(d) for d in (c, uc, c2, uc2))
    eng, L, B, seed, f = _sdxl_engine(dd8=True), meta["L"], meta["B"], meta["seed"], meta["factor"]
    L2 = int(L * f)
    enc_noise, fwd_noise = (synth_input(n, (B, 4, L2, L2), seed).to(DEV) for n in ("xllz.encnoise", "xllz.fwdnoise"))
    kw = dict(steps=meta["S"], cfg_scale=meta["cfg"])
    images, x, base = P.txt2img_sdxl_hires(eng, c, uc, height=8 * L, width=8 * L, factor=f, strength=0.5, upscaler="lanczos", c_hires=c2,
                                           uc_hires=uc2, x0=g["x0"].to(DEV), fwd_noise=fwd_noise, enc_noise=enc_noise, **kw)
    assert tuple(x.shape) == (B, 4, L2, L2) and tuple(images.shape) == (B, 3, 8 * L2, 8 * L2)
    first, base2 = P.txt2img_sdxl(eng, c, uc, height=8 * L, width=8 * L, x0=g["x0"].to(DEV), **kw)
    assert torch.equal(base2, base)
    scaled = PP.upscale_uint8(first, 8 * L2, 8 * L2).contiguous() * 2.0 - 1.0
    images2, x2 = P.img2img_sdxl(eng, scaled, c2, uc2, strength=0.5, enc_noise=enc_noise, fwd_noise=fwd_noise, **kw)
    assert torch.isfinite(x).all() and torch.equal(x2, x) and torch.equal(images2, images)
