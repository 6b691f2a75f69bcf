"""The video (SVD) UNet of cremage_amd.sgm_hip.video on a real MI355X, against fixtures made by the reference's own VideoResBlock,
VideoTransformerBlock, SpatialVideoTransformer and VideoUNet (tools/gen_golden_svd.py).  Blocks at TOL_BLOCK, nets at TOL_NET in the fp32
class (tests/test_hip_models.py).  Half type, nets: the measured rel-L2 against the fp32 fixtures is inside TOL_SDXL_BF16 for the tiny,
the small and the full-width configuration (figures in DESIGN 6 f16), so that bound is used."""
import pytest
import torch

from cremage_amd.synth import synth_fill_, synth_input
from tests.conftest import load_golden
from tests.test_hip_models import BF, DEV, TOL_BLOCK, TOL_NET, TOL_SDXL_BF16, TOL_TRAJ, close, prep

pytestmark = pytest.mark.gpu

TOL_VIDEO_HALF = TOL_SDXL_BF16
DTYPES = [torch.float32, BF]


def _indicator(meta, kind):
    b, t = meta["b"], meta["t"]
    return {"zeros": torch.zeros(b, t), "ones": torch.ones(b, t), "mixed": torch.tensor(meta["mixed"], dtype=torch.float32)}[kind].to(DEV)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("tag", ["svd_res_skip", "svd_res_same"])
def test_video_resblock(tag, dtype):
    from cremage_amd.sgm_hip.video import VideoResBlock
    meta, g = load_golden(tag)
    m = prep(VideoResBlock(meta["cin"], meta["emb_ch"], 0.0, [3, 1, 1], "learned_with_images", 0.5, meta["cout"]), meta, dtype)
    F = meta["b"] * meta["t"]
    x = synth_input(tag + ".x", (F, meta["cin"], meta["hw"], meta["hw"]), meta["seed"]).to(DEV).to(dtype).contiguous(memory_format=torch.channels_last)
    emb = synth_input(tag + ".emb", (F, meta["emb_ch"]), meta["seed"]).to(DEV).to(dtype)
    for kind in ("zeros", "ones", "mixed"):
        with torch.no_grad():
            y = m(x, emb, meta["t"], _indicator(meta, kind))
        close(y, g["y_" + kind], TOL_BLOCK[dtype], f"{tag} {kind} {dtype}")


@pytest.mark.parametrize("dtype", DTYPES)
def test_video_transformer_block(dtype):
    from cremage_amd.sgm_hip.video import VideoTransformerBlock
    tag = "svd_vtblock"
    meta, g = load_golden(tag)
    m = prep(VideoTransformerBlock(meta["dim"], meta["heads"], meta["d_head"], context_dim=meta["ctx_dim"], checkpoint=False, ff_in=True,
                                   inner_dim=meta["dim"]), meta, dtype)
    x = synth_input(tag + ".x", (meta["b"] * meta["t"], meta["s"], meta["dim"]), meta["seed"]).to(DEV).to(dtype)
    ctx = synth_input(tag + ".ctx", (meta["b"], meta["m"], meta["ctx_dim"]), meta["seed"]).to(DEV).to(dtype)
    with torch.no_grad():
        y = m(x, context=ctx, timesteps=meta["t"])
    close(y, g["y"], TOL_BLOCK[dtype], f"{tag} {dtype}")


@pytest.mark.parametrize("dtype", DTYPES)
def test_spatial_video_transformer(dtype):
    from cremage_amd.sgm_hip.video import SpatialVideoTransformer
    tag = "svd_svt"
    meta, g = load_golden(tag)
    m = prep(SpatialVideoTransformer(meta["ch"], meta["heads"], meta["d_head"], depth=1, context_dim=meta["ctx_dim"], use_spatial_context=True,
                                     use_linear=True, ff_in=True, merge_strategy="learned_with_images"), meta, dtype)
    F = meta["b"] * meta["t"]
    x = synth_input(tag + ".x", (F, meta["ch"], meta["h"], meta["w"]), meta["seed"]).to(DEV).to(dtype).contiguous(memory_format=torch.channels_last)
    ctx = synth_input(tag + ".ctx", (F, meta["m"], meta["ctx_dim"]), meta["seed"]).to(DEV).to(dtype)
    for kind in ("zeros", "ones", "mixed"):
        with torch.no_grad():
            y = m(x, context=ctx, timesteps=meta["t"], image_only_indicator=_indicator(meta, kind))
        close(y, g["y_" + kind], TOL_BLOCK[dtype], f"{tag} {kind} {dtype}")


# ---------------------------------------------------------------------------------------------------------------------------- nets
def _inputs(name, meta, videos=None):
    cfg, t = meta["cfg"], meta["t"]
    F = meta["b"] * t
    x = synth_input(name + ".x", (F, cfg["in_channels"], meta["h"], meta["w"]), meta["seed"]).to(DEV)
    ctx = synth_input(name + ".ctx", (F, 1, cfg["context_dim"]), meta["seed"]).to(DEV)
    y = synth_input(name + ".y", (F, cfg["adm_in_channels"]), meta["seed"]).to(DEV)
    return x, ctx, y


def _run(m, name, meta, g, kind="zeros", call=None):
    x, ctx, y = _inputs(name, meta)
    with torch.no_grad():
        return (call or m)(x, timesteps=g["t"].to(DEV), context=ctx, y=y, num_video_frames=meta["t"], image_only_indicator=_indicator(meta, kind))


@pytest.mark.parametrize("dtype", DTYPES)
def test_video_unet_tiny(dtype):
    from cremage_amd.sgm_hip.video import VideoUNet
    meta, g = load_golden("svd_unet_tiny")
    m = prep(VideoUNet(**meta["cfg"]), meta, dtype)
    for kind in ("zeros", "ones", "mixed"):
        r = close(_run(m, "svd_unet_tiny", meta, g, kind), g["y_" + kind], TOL_VIDEO_HALF if dtype == BF else TOL_NET[dtype], f"svd_unet_tiny {kind} {dtype}")
        print(f"\n[parity] svd_unet_tiny {kind} {dtype}: rel-L2 {r:.3e}")


@pytest.mark.parametrize("dtype", DTYPES)
def test_video_unet_small(dtype):
    from cremage_amd.sgm_hip.video import VideoUNet
    meta, g = load_golden("svd_unet_small")
    m = prep(VideoUNet(**meta["cfg"]), meta, dtype)
    r = close(_run(m, "svd_unet_small", meta, g), g["y_zeros"], TOL_VIDEO_HALF if dtype == BF else TOL_NET[dtype], f"svd_unet_small {dtype}")
    print(f"\n[parity] svd_unet_small {dtype}: rel-L2 {r:.3e}")


@pytest.fixture(scope="module")
def full_weights():
    """The full-width net's name-keyed synthetic weights (fp32, CPU): one fill for both dtypes."""
    from cremage_amd.sgm_hip.video import VideoUNet
    meta, _ = load_golden("svd_unet_full")
    with torch.device("meta"):
        m = VideoUNet(**meta["cfg"])
    return synth_fill_(m.to_empty(device="cpu"), meta["seed"], prefix=meta["prefix"]).state_dict()


@pytest.mark.parametrize("dtype", DTYPES)
def test_video_unet_full_width(dtype, full_weights):
    """svd_xt_1_1.yaml's network (model_channels 320, 2560-channel concats, 20 heads) at b = 2, T = 3, 16 x 16 latents."""
    from cremage_amd.sgm_hip.video import VideoUNet
    meta, g = load_golden("svd_unet_full")
    with torch.device("meta"):
        m = VideoUNet(**meta["cfg"])
    m = m.to_empty(device=DEV)
    m.load_state_dict(full_weights)
    m = m.to(dtype).eval()
    assert sum(p.numel() for p in m.parameters()) == meta["n_params"]
    r = close(_run(m, "svd_unet_full", meta, g), g["y_zeros"], TOL_VIDEO_HALF if dtype == BF else TOL_NET[dtype], f"svd_unet_full {dtype}")
    print(f"\n[parity] svd_unet_full {dtype}: rel-L2 {r:.3e}")


@pytest.mark.parametrize("dtype", DTYPES)
def test_all_image_frames_is_the_spatial_network(dtype):
    """An all-ones image_only_indicator switches every temporal layer off (alpha = 1): the video net must then equal the image network
    with the same spatial weights - sgm_hip.UNetModel, loaded with the video net's non-temporal keys."""
    from cremage_amd.sgm_hip.unet import UNetModel
    from cremage_amd.sgm_hip.video import VideoUNet
    meta, g = load_golden("svd_unet_tiny")
    cfg = meta["cfg"]
    m = prep(VideoUNet(**cfg), meta, dtype)
    img_cfg = {k: cfg[k] for k in ("adm_in_channels", "num_classes", "use_checkpoint", "in_channels", "out_channels", "model_channels",
                                   "attention_resolutions", "num_res_blocks", "channel_mult", "num_head_channels", "use_linear_in_transformer",
                                   "transformer_depth", "context_dim", "spatial_transformer_attn_type")}
    im = UNetModel(**img_cfg)
    temporal = (".time_stack.", ".time_mixer.", ".time_pos_embed.")
    sd = {k: v for k, v in m.state_dict().items() if not any(s in k for s in temporal)}
    assert set(sd) == set(im.state_dict())
    im.load_state_dict(sd)
    im = im.to(dtype).to(DEV).eval()
    x, ctx, y = _inputs("svd_unet_tiny", meta)
    with torch.no_grad():
        want = im(x, timesteps=g["t"].to(DEV), context=ctx, y=y)
    close(_run(m, "svd_unet_tiny", meta, g, "ones"), want.float().cpu(), TOL_BLOCK[dtype], f"video net, all image frames {dtype}")


def test_video_trajectory():
    """3-step Euler-EDM run of the tiny net with LinearPredictionGuider through pipeline.img2vid_latents, fp32 class, against the
    reference's Denoiser + VScalingWithEDMcNoise + EulerEDMSampler on EDMDiscretization(sigma_max 700)."""
    from cremage_amd import pipeline
    from cremage_amd.sgm_hip.video import VideoUNet
    meta, g = load_golden("svd_traj")
    cfg = meta["cfg"]
    m = prep(VideoUNet(**cfg), meta, torch.float32)
    F = meta["b"] * meta["t"]

    def cond(tag):
        return {"crossattn": synth_input(f"svd_traj.{tag}.ctx", (F, 1, cfg["context_dim"]), meta["seed"]).to(DEV),
                "vector": synth_input(f"svd_traj.{tag}.y", (F, cfg["adm_in_channels"]), meta["seed"]).to(DEV),
                "concat": synth_input(f"svd_traj.{tag}.cat", (F, 4, meta["h"], meta["w"]), meta["seed"]).to(DEV)}
    x = synth_input("svd_traj.x", (F, 4, meta["h"], meta["w"]), meta["seed"]).to(DEV)
    z = pipeline.img2vid_latents(m, cond("c"), cond("uc"), num_frames=meta["t"], steps=meta["steps"], min_scale=meta["min_scale"],
                                 max_scale=meta["max_scale"], x0=x, sigma_max=meta["sigma_max"])
    close(z, g["z"], TOL_TRAJ, "svd trajectory fp32")


@pytest.mark.parametrize("dtype", DTYPES)
def test_video_unet_graph_replay_is_eager(dtype):
    from cremage_amd.graphs import GraphedModule
    from cremage_amd.sgm_hip.video import VideoUNet
    meta, g = load_golden("svd_unet_tiny")
    m = prep(VideoUNet(**meta["cfg"]), meta, dtype)
    gm = GraphedModule(m, scratch_bytes=64 << 20)
    x, ctx, y = _inputs("svd_unet_tiny", meta)
    kw = dict(context=ctx, y=y, num_video_frames=meta["t"])
    with torch.no_grad():
        for kind in ("mixed", "zeros"):  # the indicator is a dynamic input: the second call replays the first one's graph
            ind = _indicator(meta, kind)
            eager = m(x, timesteps=g["t"].to(DEV), image_only_indicator=ind, **kw)
            assert torch.equal(gm(x, timesteps=g["t"].to(DEV), image_only_indicator=ind, **kw), eager)
    assert gm.captures == 1 and gm.replays == 1


@pytest.mark.parametrize("dtype", DTYPES)
def test_video_unet_batch_invariant(dtype):
    """Under the batch-invariant mode video 0 of a batch of two has the bits of video 0 run alone."""
    import cremage_amd
    from cremage_amd.sgm_hip.video import VideoUNet
    meta, g = load_golden("svd_unet_tiny")
    m = prep(VideoUNet(**meta["cfg"]), meta, dtype)
    x, ctx, y = _inputs("svd_unet_tiny", meta)
    t, T = g["t"].to(DEV), meta["t"]
    ind = _indicator(meta, "mixed")
    cremage_amd.set_batch_invariant(8)
    try:
        with torch.no_grad():
            both = m(x, timesteps=t, context=ctx, y=y, num_video_frames=T, image_only_indicator=ind)
            solo = m(x[:T].clone(), timesteps=t[:T].clone(), context=ctx[:T].clone(), y=y[:T].clone(), num_video_frames=T,
                     image_only_indicator=ind[:1].clone())
    finally:
        cremage_amd.set_batch_invariant(None)
    assert torch.equal(both[:T], solo)
