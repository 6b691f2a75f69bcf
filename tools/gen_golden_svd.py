"""ORACLE tooling for the video (SVD) UNet - writes tests/golden/svd_*.npz from the reference's own modules (sgm VideoResBlock,
VideoTransformerBlock, SpatialVideoTransformer and VideoUNet at the svd_xt_1_1.yaml settings), on the name-keyed synthetic weights and
`synth_input` tensors of oracle/gen_golden.py, whose import stubs and helpers it reuses (that module is imported, not changed).
The reference's "softmax-xformers" attention needs xformers; the fixtures are generated with "softmax", the same arithmetic.
Only the .npz files are committed; a rerun reproduces them exactly (apart from timing meta).

    python tools/gen_golden_svd.py [--only NAME ...] [--skip-full]
"""
import argparse
import hashlib
import os
import sys
import time

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from oracle import gen_golden as G  # noqa: E402  (installs the import stubs and puts the reference on sys.path)
from oracle.gen_golden import SEED, fp32_forward, save, synth_fill_, synth_input  # noqa: E402

# svd_xt_1_1.yaml network params (use_checkpoint only selects activation checkpointing for training; attention type: see above)
SVD_XT_UNET = dict(adm_in_channels=768, num_classes="sequential", use_checkpoint=False, in_channels=8, out_channels=4, model_channels=320,
                   attention_resolutions=[4, 2, 1], num_res_blocks=2, channel_mult=[1, 2, 4, 4], num_head_channels=64,
                   use_linear_in_transformer=True, transformer_depth=1, context_dim=1024, spatial_transformer_attn_type="softmax",
                   extra_ff_mix_layer=True, use_spatial_context=True, merge_strategy="learned_with_images", video_kernel_size=[3, 1, 1])
TINY_SVD_UNET = dict(SVD_XT_UNET, adm_in_channels=48, model_channels=32, attention_resolutions=[2, 1], num_res_blocks=1, channel_mult=[1, 2],
                     num_head_channels=16, context_dim=64)
SMALL_SVD_UNET = dict(SVD_XT_UNET, adm_in_channels=96, model_channels=64, num_head_channels=32, context_dim=128)
MIXED = {3: [[0, 1, 0], [1, 0, 0]], 5: [[0, 0, 1, 0, 1], [1, 0, 0, 0, 0]]}


def _video_modules():
    G._import_sgm()
    from sgm.modules import video_attention
    from sgm.modules.diffusionmodules import video_model
    return video_model, video_attention


def _key_digest(module):
    items = sorted(f"{k}:{tuple(v.shape)}" for k, v in module.state_dict().items())
    return hashlib.sha1("\n".join(items).encode()).hexdigest(), len(items)


def _indicators(b, t):
    return dict(zeros=torch.zeros(b, t), ones=torch.ones(b, t), mixed=torch.tensor(MIXED[t], dtype=torch.float32))


def g_resblock():
    VM, _ = _video_modules()
    b, t, hw, emb_ch = 2, 3, 8, 128
    for tag, cin, cout in [("svd_res_skip", 64, 96), ("svd_res_same", 64, None)]:
        m = VM.VideoResBlock(channels=cin, emb_channels=emb_ch, dropout=0.0, video_kernel_size=[3, 1, 1], merge_strategy="learned_with_images",
                             merge_factor=0.5, out_channels=cout)
        synth_fill_(m, SEED, prefix=tag + ".")
        x = synth_input(tag + ".x", (b * t, cin, hw, hw), SEED)
        emb = synth_input(tag + ".emb", (b * t, emb_ch), SEED)
        outs = {}
        with fp32_forward():
            for k, ind in _indicators(b, t).items():
                outs["y_" + k] = m(x, emb, t, ind)
        sha, n = _key_digest(m)
        save(tag, dict(cin=cin, cout=cout, emb_ch=emb_ch, b=b, t=t, hw=hw, seed=SEED, prefix=tag + ".", n_keys=n, keys_sha1=sha, mixed=MIXED[t]), **outs)


def g_vtblock():
    _, VA = _video_modules()
    tag, b, t, s, dim, heads, dh, cdim, mk = "svd_vtblock", 2, 3, 20, 64, 4, 16, 48, 2
    m = VA.VideoTransformerBlock(dim, heads, dh, context_dim=cdim, checkpoint=False, ff_in=True, inner_dim=dim, attn_mode="softmax")
    synth_fill_(m, SEED, prefix=tag + ".")
    x = synth_input(tag + ".x", (b * t, s, dim), SEED)
    ctx = synth_input(tag + ".ctx", (b, mk, cdim), SEED)  # one context per video; the reference wants it repeated over the pixels
    with fp32_forward():
        y = m(x, context=ctx.repeat_interleave(s, dim=0), timesteps=t)
    sha, n = _key_digest(m)
    save(tag, dict(b=b, t=t, s=s, dim=dim, heads=heads, d_head=dh, ctx_dim=cdim, m=mk, seed=SEED, prefix=tag + ".", n_keys=n, keys_sha1=sha), y=y)


def g_svt():
    _, VA = _video_modules()
    tag, b, t, h, w, ch, heads, dh, cdim, mk = "svd_svt", 2, 3, 4, 5, 64, 4, 16, 48, 3
    m = VA.SpatialVideoTransformer(ch, heads, dh, depth=1, context_dim=cdim, use_spatial_context=True, use_linear=True, ff_in=True,
                                   merge_strategy="learned_with_images", checkpoint=False, attn_mode="softmax")
    synth_fill_(m, SEED, prefix=tag + ".")
    x = synth_input(tag + ".x", (b * t, ch, h, w), SEED)
    ctx = synth_input(tag + ".ctx", (b * t, mk, cdim), SEED)
    outs = {}
    with fp32_forward():
        for k, ind in _indicators(b, t).items():
            outs["y_" + k] = m(x, context=ctx, timesteps=t, image_only_indicator=ind)
    sha, n = _key_digest(m)
    save(tag, dict(b=b, t=t, h=h, w=w, ch=ch, heads=heads, d_head=dh, ctx_dim=cdim, m=mk, seed=SEED, prefix=tag + ".", n_keys=n, keys_sha1=sha,
                   mixed=MIXED[t]), **outs)


def _unet_case(name, cfg, b, t, h, w, tvals, kinds=("zeros",)):
    VM, _ = _video_modules()
    m = VM.VideoUNet(**cfg)
    synth_fill_(m, SEED, prefix="svd_unet.")
    F = b * t
    x = synth_input(name + ".x", (F, cfg["in_channels"], h, w), SEED)
    ctx = synth_input(name + ".ctx", (F, 1, cfg["context_dim"]), SEED)
    y = synth_input(name + ".y", (F, cfg["adm_in_channels"]), SEED)
    tt = torch.tensor(tvals, dtype=torch.float32).repeat_interleave(t)  # one sigma per video, as the sampler hands it over
    outs, t0 = {}, time.time()
    with fp32_forward():
        for k in kinds:
            outs["y_" + k] = m(x, timesteps=tt, context=ctx, y=y, num_video_frames=t, image_only_indicator=_indicators(b, t)[k])
    sha, n = _key_digest(m)
    n_t = sum(1 for k in m.state_dict() if ".time_stack." in k or ".time_mixer." in k or ".time_pos_embed." in k)
    save(name, dict(cfg=cfg, b=b, t=t, h=h, w=w, seed=SEED, prefix="svd_unet.", n_params=sum(p.numel() for p in m.parameters()), n_keys=n,
                    n_temporal_keys=n_t, keys_sha1=sha, ref_cpu_seconds=time.time() - t0, threads=torch.get_num_threads(),
                    mixed=MIXED.get(t)), t=tt, **outs)


def g_unet_tiny():
    _unet_case("svd_unet_tiny", TINY_SVD_UNET, 2, 3, 8, 16, [-1.5, 0.7], kinds=("zeros", "ones", "mixed"))


def g_unet_small():
    _unet_case("svd_unet_small", SMALL_SVD_UNET, 2, 5, 16, 16, [0.3, -2.0])


def g_unet_full():
    # the full SVD-XT configuration at reduced extent: every real channel width (2560-channel concats, 20 heads) at 16 x 16 latents
    _unet_case("svd_unet_full", SVD_XT_UNET, 2, 3, 16, 16, [1.1, -0.9])


TRAJ = dict(b=1, t=3, h=8, w=16, steps=3, min_scale=1.0, max_scale=2.5, sigma_max=700.0)


def g_tables():
    """VScalingWithEDMcNoise over a sigma grid, LinearPredictionGuider's scale rows and the EDM sigmas of svd_xt_1_1.yaml's sampler"""
    _, _, DZ, GD, _, _ = G._import_sgm()
    from sgm.modules.diffusionmodules import denoiser_scaling
    sig = torch.tensor([0.002, 0.05, 0.7, 1.0, 3.5, 80.0, 700.0])
    cs = denoiser_scaling.VScalingWithEDMcNoise()(sig)
    arrays = dict(sigma=sig, c_skip=cs[0], c_out=cs[1], c_in=cs[2], c_noise=cs[3])
    for t in (14, 25):
        arrays[f"scale_{t}"] = GD.LinearPredictionGuider(max_scale=2.5, num_frames=t, min_scale=1.0).scale
    arrays["scale_3_0"] = GD.LinearPredictionGuider(max_scale=3.0, num_frames=21, min_scale=1.5).scale
    for n in (3, 25, 30):
        arrays[f"edm_{n}"] = DZ.EDMDiscretization(sigma_max=700.0)(n)
    save("svd_tables", dict(seed=SEED), **arrays)


def g_traj():
    """3-step Euler-EDM trajectory of the tiny net: reference Denoiser + VScalingWithEDMcNoise + LinearPredictionGuider + EulerEDMSampler"""
    import types
    VM, _ = _video_modules()
    _, DN, DZ, GD, SM, WR = G._import_sgm()
    SM.denoising_status_queue = types.SimpleNamespace(put=lambda *a, **k: None)
    p, cfg = TRAJ, TINY_SVD_UNET
    m = VM.VideoUNet(**cfg)
    synth_fill_(m, SEED, prefix="svd_unet.")
    F = p["b"] * p["t"]

    def cond(tag):
        return {"crossattn": synth_input(f"svd_traj.{tag}.ctx", (F, 1, cfg["context_dim"]), SEED),
                "vector": synth_input(f"svd_traj.{tag}.y", (F, cfg["adm_in_channels"]), SEED),
                "concat": synth_input(f"svd_traj.{tag}.cat", (F, 4, p["h"], p["w"]), SEED)}
    c, uc = cond("c"), cond("uc")
    x = synth_input("svd_traj.x", (F, 4, p["h"], p["w"]), SEED)
    den = DN.Denoiser(scaling_config={"target": "sgm.modules.diffusionmodules.denoiser_scaling.VScalingWithEDMcNoise"})
    net = WR.OpenAIWrapper(m)
    sampler = SM.EulerEDMSampler(discretization_config={"target": "sgm.modules.diffusionmodules.discretizer.EDMDiscretization",
                                                        "params": {"sigma_max": p["sigma_max"]}},
                                 num_steps=p["steps"], verbose=False, device="cpu",
                                 guider_config={"target": "sgm.modules.diffusionmodules.guiders.LinearPredictionGuider",
                                                "params": {"max_scale": p["max_scale"], "min_scale": p["min_scale"], "num_frames": p["t"]}})
    extra = dict(image_only_indicator=torch.zeros(2 * p["b"], p["t"]), num_video_frames=p["t"])
    with fp32_forward():
        z = sampler(lambda inp, sigma, cc: den(net, inp, sigma, cc, **extra), x.clone(), cond=c, uc=uc)
    sha, n = _key_digest(m)
    save("svd_traj", dict(cfg=cfg, seed=SEED, prefix="svd_unet.", n_keys=n, keys_sha1=sha, **p), z=z)


ALL = dict(tables=g_tables, traj=g_traj, resblock=g_resblock, vtblock=g_vtblock, svt=g_svt, unet_tiny=g_unet_tiny, unet_small=g_unet_small, unet_full=g_unet_full)

if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", nargs="*", default=None)
    ap.add_argument("--skip-full", action="store_true")
    a = ap.parse_args()
    torch.manual_seed(0)
    for key, fn in ALL.items():
        if (a.only and key not in a.only) or (a.skip_full and key == "unet_full"):
            continue
        fn()
