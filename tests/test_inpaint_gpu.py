"""SD1.5 inpainting on a real MI355X: the 9-channel UNet (conv_in on the thin-input conv with the c_concat planes folded into the
input conversion) and the eta = 1 DDIM trajectory against the reference's own modules (tests/golden/inpaint_*.npz,
tests/golden/traj_inpaint_ddim.npz written by tools/gen_golden_inpaint.py), the CFG-shared prefix and hipGraph replay with
c_concat, and the two new kernels against fp32 CPU arithmetic."""
import pytest
import torch
import torch.nn.functional as F

from cremage_amd.synth import synth_input
from tests.conftest import load_golden
from tests.test_hip_models import BF, DEV, TOL_BLOCK, TOL_NET, TOL_TRAJ, close, prep

pytestmark = pytest.mark.gpu


def _unet_case(name, dtype):
    from cremage_amd.ldm_hip.unet import UNetModel
    meta, g = load_golden(name)
    cfg = meta["cfg"]
    m = UNetModel(**cfg)
    assert sum(p.numel() for p in m.parameters()) == meta["n_params"]
    m = prep(m, meta, dtype)
    x = synth_input(name + ".x", (meta["B"], 9, meta["L"], meta["L"]), meta["seed"]).to(DEV)
    ctx = synth_input(name + ".ctx", (meta["B"], meta["m"], cfg["context_dim"]), meta["seed"]).to(DEV)
    t = g["t"].to(DEV)
    with torch.no_grad():
        y = m(x, timesteps=t, context=ctx)
        y_cc = m(x[:, :4].contiguous(), timesteps=t, context=ctx, c_concat=x[:, 4:].contiguous())
    assert y.dtype == torch.float32 and y.is_contiguous()
    close(y, g["y"], TOL_NET[dtype], name)
    assert torch.equal(y, y_cc), name  # the concat folded into the input conversion is the same input


@pytest.mark.parametrize("dtype", [torch.float32, BF])
@pytest.mark.parametrize("name", ["inpaint_unet_tiny", "inpaint_unet_small_sd"])
def test_inpaint_unet_small(dtype, name):
    _unet_case(name, dtype)


@pytest.mark.parametrize("dtype", [torch.float32, BF])
def test_inpaint_unet_sd15_full(dtype):
    """The SD1.5 inpainting UNet (inpainting.yaml: 9 input channels), B=2, 64x64 latent, against the reference's UNetModel."""
    _unet_case("inpaint_unet_sd15_full", dtype)


def _traj_setup():
    from cremage_amd import pipeline as P
    meta, g = load_golden("traj_inpaint_ddim")
    ldm = P.build_synthetic_inpaint_ldm(meta["unet"], meta["dd"], DEV, unet_dtype=torch.float32, vae_dtype=torch.float32, seed=meta["seed"])
    B, L, HW, seed = meta["B"], meta["L"], meta["HW"], meta["seed"]
    inp = dict(c=synth_input("inpaint.c", (B, 77, 96), seed), uc=synth_input("inpaint.uc", (B, 77, 96), seed),
               image=synth_input("inpaint.img", (B, 3, HW, HW), seed, 0.5).clamp(-1, 1),
               mask=(synth_input("inpaint.mask", (B, 1, HW, HW), seed) > meta["mask_threshold"]).float(),
               enc_noise=synth_input("inpaint.encnoise", (B, 4, L, L), seed))
    inp = {k: v.to(DEV) for k, v in inp.items()}
    calls = []

    def noise_sampler(sigma, index):  # ddim.noise_like of the reference run, step by step
        z = synth_input(f"inpaint.noise{len(calls)}", (B, 4, L, L), seed).to(DEV)
        calls.append(index)
        return z
    return meta, g, ldm, inp, noise_sampler, calls


def test_inpaint_trajectory_through_pipeline():
    from cremage_amd import pipeline as P
    meta, g, ldm, inp, ns, calls = _traj_setup()
    images, x = P.inpaint(ldm, inp["image"], inp["mask"], inp["c"], inp["uc"], steps=meta["S"], cfg_scale=meta["cfg"], eta=meta["eta"],
                          seed=meta["seed"], noise_sampler=ns, enc_noise=inp["enc_noise"])
    assert len(calls) == meta["S"]
    close(x, g["x"], TOL_TRAJ, "inpaint ddim latent")
    ref_img = ((g["img"] + 1) / 2).clamp(0, 1)
    assert (images.cpu() - ref_img).abs().max().item() < 2e-3


def test_inpaint_trajectory_through_sampler_fused_and_chain():
    """DDIMSampler.sample alone from the reference's c_concat and start code: the fused step (crg_cfg_ddim_step) and, with a callback,
    the elementwise chain of p_sample_ddim."""
    from cremage_amd.samplers import DDIMSampler
    meta, g, ldm, inp, ns, calls = _traj_setup()
    B, L = meta["B"], meta["L"]
    c_cat = g["c_cat"].to(DEV)
    cond = {"c_concat": [c_cat], "c_crossattn": [inp["c"]]}
    uc = {"c_concat": [c_cat], "c_crossattn": [inp["uc"]]}
    x, _ = DDIMSampler(ldm).sample(meta["S"], B, [4, L, L], cond, eta=meta["eta"], x_T=g["start"].to(DEV),
                                   unconditional_guidance_scale=meta["cfg"], unconditional_conditioning=uc, noise_sampler=ns)
    close(x, g["x"], TOL_TRAJ, "inpaint ddim latent (sampler, fused)")
    calls.clear()
    seen = []
    x2, _ = DDIMSampler(ldm).sample(meta["S"], B, [4, L, L], cond, eta=meta["eta"], x_T=g["start"].to(DEV),
                                    unconditional_guidance_scale=meta["cfg"], unconditional_conditioning=uc, noise_sampler=ns,
                                    callback=seen.append)
    assert seen == list(range(meta["S"]))
    close(x2, g["x"], TOL_TRAJ, "inpaint ddim latent (sampler, chain)")


@pytest.mark.parametrize("dtype", [torch.float32, BF])
def test_cfg_shared_prefix_with_c_concat(dtype):
    from cremage_amd import ops
    from cremage_amd.ldm_hip.latent_diffusion import DiffusionWrapper
    from cremage_amd.ldm_hip.unet import UNetModel
    from cremage_amd.samplers import cat_cond_dict
    meta, _ = load_golden("inpaint_unet_small_sd")
    cfg = meta["cfg"]
    m = prep(UNetModel(**cfg), meta, dtype)
    xh = synth_input("cfgcc.x", (2, 4, 16, 16), 5).to(DEV)
    cch = synth_input("cfgcc.cc", (2, 5, 16, 16), 6).to(DEV)
    x = torch.cat([xh, xh])
    t = torch.tensor([801.5, 333.25, 801.5, 333.25], device=DEV)
    ctx = synth_input("cfgcc.ctx", (4, 77, cfg["context_dim"]), 7).to(DEV)
    # the sampler's rule: one c_concat object in both dicts -> marked; equal values in two objects -> not marked
    same = cat_cond_dict({"c_concat": [cch], "c_crossattn": [ctx[2:]]}, {"c_concat": [cch], "c_crossattn": [ctx[:2]]})
    other = cat_cond_dict({"c_concat": [cch], "c_crossattn": [ctx[2:]]}, {"c_concat": [cch.clone()], "c_crossattn": [ctx[:2]]})
    assert getattr(same["c_concat"][0], "_crg_cfg_dup", False) and not getattr(other["c_concat"][0], "_crg_cfg_dup", False)
    assert torch.equal(same["c_crossattn"][0], ctx)
    cc_marked, cc_plain = same["c_concat"][0], other["c_concat"][0]
    with torch.no_grad():
        full = m(x.clone(), timesteps=t, context=ctx, c_concat=cc_plain)
        shared = m(ops.mark_cfg_dup(x.clone()), timesteps=t, context=ctx, c_concat=cc_marked)
        unmarked_cc = m(ops.mark_cfg_dup(x.clone()), timesteps=t, context=ctx, c_concat=cc_plain)
        ref = m(torch.cat([x, cc_plain], 1), timesteps=t, context=ctx)
    close(shared, full.float().cpu(), TOL_BLOCK[dtype], "cfg-shared prefix with c_concat vs full batch")
    assert torch.equal(unmarked_cc, full) and torch.equal(ref, full)
    # hipGraph replay through the hybrid wrapper: c_concat is a constant argument keyed on identity + version
    w = DiffusionWrapper(m, "hybrid")
    w.enable_hip_graph()
    w.graphed.scratch_bytes = 64 << 20
    with torch.no_grad():
        g1 = w(ops.mark_cfg_dup(x.clone()), t, c_concat=[cc_marked], c_crossattn=[ctx])  # captures
        g2 = w(ops.mark_cfg_dup(x.clone()), t, c_concat=[cc_marked], c_crossattn=[ctx])  # replays
        assert w.graphed.captures == 1 and w.graphed.replays == 1
        cc_new = ops.mark_cfg_dup(torch.cat([cch.flip(-1)] * 2))
        g3 = w(ops.mark_cfg_dup(x.clone()), t, c_concat=[cc_new], c_crossattn=[ctx])
        e3 = m(ops.mark_cfg_dup(x.clone()), timesteps=t, context=ctx, c_concat=cc_new)
    assert torch.equal(g1, shared) and torch.equal(g2, shared)
    assert w.graphed.captures == 2 and torch.equal(g3, e3) and not torch.equal(g3, g1)


@pytest.mark.parametrize("dtype", [torch.float32, BF])
@pytest.mark.parametrize("shape", [(2, 64, 64), (3, 13, 21), (1, 12, 20)])
def test_conv_in_nine_channels_one_and_two_source(dtype, shape):
    """The thin-input 3x3 conv at Cin = 9 (one NHWC source, and the 4 + 5 planes joined by the input conversion) against F.conv2d in fp32
    on the CPU: the full-size conv_in shape (320 outputs, 64x64) and odd sizes (widths that are not a multiple of 4 take one pixel per
    thread)."""
    from cremage_amd import ops
    n, h, w = shape
    x = synth_input("cin9.x", (n, 4, h, w), 1)
    cc = synth_input("cin9.cc", (n, 5, h, w), 2)
    wt = synth_input("cin9.w", (320, 9, 3, 3), 3, 1 / 9)
    b = synth_input("cin9.b", (320,), 4, 0.05)
    ref = F.conv2d(torch.cat([x, cc], 1).to(dtype).float(), wt.to(dtype).float(), b.to(dtype).float(), padding=1)
    wd, bd = wt.to(dtype).to(DEV), b.to(dtype).to(DEV)
    one = ops.conv2d(ops.nchw_to_nhwc(torch.cat([x, cc], 1).to(DEV), dtype), wd, bd)
    two = ops.conv2d(ops.nchw_to_nhwc(x.to(DEV), dtype, cc.to(DEV)), wd, bd)
    assert one.dtype == dtype and one.shape == (n, 320, h, w)
    assert torch.equal(one, two)
    tol = 1e-5 if dtype == torch.float32 else 8e-3
    err = (one.float().cpu() - ref).abs().max().item() / ref.abs().max().item()
    assert err < tol, err


@pytest.mark.parametrize("cfg", [1.0, 7.5])
@pytest.mark.parametrize("eta", [0.0, 1.0])
def test_cfg_ddim_step_matches_elementwise_chain(cfg, eta):
    """crg_cfg_ddim_step against p_sample_ddim's elementwise chain in fp32 on the CPU, with the sampler's own per-step scalars."""
    from cremage_amd import ops
    from cremage_amd.samplers import DDIMSampler, make_alphas_cumprod

    class M:
        num_timesteps = 1000
        alphas_cumprod = make_alphas_cumprod(1000)
        device = torch.device("cpu")
    s = DDIMSampler(M())
    s.make_schedule(20, ddim_eta=eta)
    x = synth_input("ddimstep.x", (2, 4, 24, 40), 1)
    eps = synth_input("ddimstep.eps", (4, 4, 24, 40), 2)
    z = synth_input("ddimstep.z", (2, 4, 24, 40), 3)
    for index in (19, 7, 0):
        sq1ma, sqa, sqap, dirc, sig = s._step_scalars[index]
        eu, ec = eps[:2], eps[2:]
        e = eu + cfg * (ec - eu)
        x0 = (x - torch.tensor(sq1ma) * e) / torch.tensor(sqa)
        ref = torch.tensor(sqap) * x0 + torch.tensor(dirc) * e
        if sig != 0.0:
            ref = ref + torch.tensor(sig) * z
        got = x.to(DEV).contiguous()
        ops.cfg_ddim_step_(got, eps.to(DEV).contiguous(), z.to(DEV).contiguous(), cfg, sq1ma, sqa, sqap, dirc, sig)
        d = (got.cpu() - ref).abs().max().item()
        assert d <= 1e-6 * ref.abs().max().item(), (index, d)
        # sigma = 0 reads no noise: a NaN noise tensor must not reach the result
        if sig == 0.0:
            got2 = x.to(DEV).contiguous()
            ops.cfg_ddim_step_(got2, eps.to(DEV).contiguous(), torch.full_like(got2, float("nan")), cfg, sq1ma, sqa, sqap, dirc, 0.0)
            assert torch.equal(got2, got)
