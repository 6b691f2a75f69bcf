"""CPU-side checks of the video (SVD) path: the address arithmetic of cremage_amd/csrc/video.hip restated on the host and held inside
its operands for every shape tests/test_svd_ops_gpu.py launches, and the ABI surface of the new entry points."""
import re
from pathlib import Path

import numpy as np
import pytest

from tests._svd_cases import ATTN_CASES, CONV_CASES, attn_frames_offsets, conv_frames_offsets

ROOT = Path(__file__).resolve().parents[1]


@pytest.mark.parametrize("b,T,S,Cin,Cout", CONV_CASES + [(1, 1, 1, 32, 32), (3, 2, 129, 96, 96), (2, 32, 127, 32, 160)])
def test_conv_frames_addresses(b, T, S, Cin, Cout):
    o = conv_frames_offsets(b, T, S, Cin, Cout)
    M, N, K = o["M"], o["N"], o["K"]
    sel, off, tap = o["x_sel"], o["x_off"], o["tap"]
    assert sel.any()
    # every selected 16-byte piece (8 elements) lies inside x ...
    assert (off[sel] >= 0).all() and (off[sel] + 8 <= M * Cin).all()
    # ... inside ONE row, and that row is the tile row shifted by (tap - 1) frames of the SAME video
    src_row = off[sel] // Cin
    assert ((off[sel] + 7) // Cin == src_row).all()
    m = np.broadcast_to(o["m"][:, None], sel.shape)[sel]
    assert (src_row == m + (tap[sel] - 1) * S).all()
    assert (src_row // (T * S) == m // (T * S)).all()
    assert (tap[sel] <= 2).all()
    # all three taps of an interior frame are read, the outer ones of a video's first / last frame are not
    fr = (m // S) % T
    assert not ((tap[sel] == 0) & (fr == 0)).any() and not ((tap[sel] == 2) & (fr == T - 1)).any()
    want = sum(int(((o["m"] < M) & ok).sum()) for ok in ((o["m"] // S % T > 0), np.ones_like(o["m"], bool), (o["m"] // S % T < T - 1))) * (Cin // 8)
    assert int(sel.sum()) == want
    # the running (tap, channel) of a lane is the division it replaces
    kc = np.arange(sel.shape[1]) * 8
    assert (tap[0][o["kok"]] == (kc // Cin)[o["kok"]]).all()
    # weights
    assert (o["w_off"][o["w_sel"]] + 8 <= N * K).all() and int(o["w_sel"].sum()) == N * (K // 8)
    # LDS: DMA pieces and fragment reads inside their halves of a stage, two stages inside the allocation
    assert o["x_dma_end"] <= o["xs_bytes"] and o["w_dma_end"] <= o["stage_bytes"] and o["x_read_end"] <= o["xs_bytes"]
    assert o["lds_bytes"] <= 64 * 1024
    assert o["y_end"] == M * N


@pytest.mark.parametrize("esize", [2, 4])
@pytest.mark.parametrize("b,T,S,H,d", ATTN_CASES + [(2, 7, 1, 3, 8), (1, 31, 5, 2, 24), (1, 32, 300, 20, 64)])
def test_attention_frames_addresses(b, T, S, H, d, esize):
    C = H * d
    ld = 3 * C  # q | k | v slices of one projection output: offsets are relative to the slice's first column
    rows_total = b * T * S
    seen_q = 0
    for blk in attn_frames_offsets(b, T, S, H, d, esize, ld):
        for off, rws in ((blk["q_off"], blk["q_rows"]), (blk["kv_off"], blk["kv_rows"])):
            assert (off >= 0).all() and (rws < rows_total).all()
            # a piece stays inside the C columns of its row's slice, and every row belongs to the block's own video
            assert (off % ld + (8 if off is blk["q_off"] else blk["epp"]) <= C).all()
            assert (rws // (T * S) == blk["video"]).all()
        assert (blk["lds_st_end"] <= blk["lds"]).all() and (blk["lds_rd_end"] <= blk["lds"]).all()
        assert blk["lds"] <= 2 * 256 * (64 * esize + 16) <= 160 * 1024
        # nothing is read from LDS that was not staged
        assert set(blk["read_rows"]) <= set(blk["staged_rows"])
        seen_q += blk["q_off"].shape[0]
    assert seen_q == rows_total * H  # every (row, head) is computed exactly once


def _digest(module):
    import hashlib
    items = sorted(f"{k}:{tuple(v.shape)}" for k, v in module.state_dict().items())
    return hashlib.sha1("\n".join(items).encode()).hexdigest(), len(items)


@pytest.mark.parametrize("name", ["svd_unet_tiny", "svd_unet_small", "svd_unet_full"])
def test_video_unet_state_dict_keys(name):
    """same module tree and parameter names / shapes as the reference's VideoUNet: digest and count of the state-dict keys"""
    import torch
    from cremage_amd.sgm_hip.video import VideoUNet
    from tests.conftest import load_golden
    meta, _ = load_golden(name)
    with torch.device("meta"):
        m = VideoUNet(**meta["cfg"])
    sha, n = _digest(m)
    assert n == meta["n_keys"] and sha == meta["keys_sha1"]
    assert sum(p.numel() for p in m.parameters()) == meta["n_params"]
    temporal = sum(1 for k in m.state_dict() if ".time_stack." in k or ".time_mixer." in k or ".time_pos_embed." in k)
    assert temporal == meta["n_temporal_keys"] > 0


@pytest.mark.parametrize("name,build", [
    ("svd_res_skip", lambda v, m: v.VideoResBlock(m["cin"], m["emb_ch"], 0.0, [3, 1, 1], "learned_with_images", 0.5, m["cout"])),
    ("svd_vtblock", lambda v, m: v.VideoTransformerBlock(m["dim"], m["heads"], m["d_head"], context_dim=m["ctx_dim"], checkpoint=False, ff_in=True,
                                                         inner_dim=m["dim"])),
    ("svd_svt", lambda v, m: v.SpatialVideoTransformer(m["ch"], m["heads"], m["d_head"], depth=1, context_dim=m["ctx_dim"], use_spatial_context=True,
                                                       use_linear=True, ff_in=True, merge_strategy="learned_with_images"))])
def test_video_block_state_dict_keys(name, build):
    from cremage_amd.sgm_hip import video
    from tests.conftest import load_golden
    meta, _ = load_golden(name)
    sha, n = _digest(build(video, meta))
    assert n == meta["n_keys"] and sha == meta["keys_sha1"]


def test_alpha_blender_get_alpha():
    import torch
    from cremage_amd.sgm_hip.video import AlphaBlender
    ind = torch.tensor([[0, 1, 0], [1, 0, 0]], dtype=torch.float32)
    s = torch.sigmoid(torch.tensor([0.3]))
    fixed = AlphaBlender(0.3, "fixed")
    assert "mix_factor" in dict(fixed.named_buffers()) and torch.equal(fixed.get_alpha(ind), torch.tensor([0.3]))
    learned = AlphaBlender(0.3, "learned")
    assert "mix_factor" in dict(learned.named_parameters()) and torch.equal(learned.get_alpha(None), s)
    want = torch.where(ind.bool(), torch.ones(()), s)
    for pattern, shape in (("b t -> (b t) 1 1", (6, 1, 1)), ("b t -> b 1 t 1 1", (2, 1, 3, 1, 1))):
        lwi = AlphaBlender(0.3, "learned_with_images", pattern)
        a = lwi.get_alpha(ind)
        assert a.shape == shape and torch.equal(a.reshape(2, 3), want)
        assert torch.equal(lwi.frame_alpha(ind, 6), want.reshape(6))  # (b t) order whichever pattern
    assert torch.equal(fixed.frame_alpha(None, 6), torch.full((6,), 0.3))
    with pytest.raises(ValueError):
        AlphaBlender(0.3, "nope")


def test_video_unet_unsupported_options_raise():
    from cremage_amd.sgm_hip.video import VideoUNet
    from tests.conftest import load_golden
    cfg = load_golden("svd_unet_tiny")[0]["cfg"]
    for bad in (dict(time_downup=True), dict(resblock_updown=True), dict(use_scale_shift_norm=True), dict(dims=3), dict(num_classes="timestep"),
                dict(video_kernel_size=3), dict(conv_resample=False), dict(max_ddpm_temb_period=100)):
        with pytest.raises(NotImplementedError):
            VideoUNet(**dict(cfg, **bad))


def test_video_sampling_tables_are_the_references():
    """VScalingWithEDMcNoise, LinearPredictionGuider's scale row and the EDM sigmas: bit-equal to what the reference's classes gave"""
    import torch
    from cremage_amd.sgm_hip.video_sampling import EulerEDMVideoSampler, LinearPredictionGuider, VScalingWithEDMcNoise
    from tests.conftest import load_golden
    _, g = load_golden("svd_tables")
    for got, name in zip(VScalingWithEDMcNoise()(g["sigma"]), ("c_skip", "c_out", "c_in", "c_noise")):
        assert torch.equal(got, g[name]), name
    for t in (14, 25):
        assert torch.equal(LinearPredictionGuider(2.5, t, 1.0).scale, g[f"scale_{t}"])
    assert torch.equal(LinearPredictionGuider(3.0, 21, 1.5).scale, g["scale_3_0"])
    for n in (3, 25, 30):
        s = EulerEDMVideoSampler(n, LinearPredictionGuider(2.5, 25), device="cpu")
        assert torch.equal(s.discretization(n, device="cpu"), g[f"edm_{n}"])


def test_linear_prediction_guider_scales_each_frame():
    import torch
    from cremage_amd.sgm_hip.video_sampling import LinearPredictionGuider
    gd = LinearPredictionGuider(3.0, 3, 1.0)
    x_u, x_c = torch.zeros(6, 4, 2, 2), torch.ones(6, 4, 2, 2)
    out = gd(torch.cat([x_u, x_c]), None)
    assert torch.equal(out[:, 0, 0, 0], torch.tensor([1.0, 2.0, 3.0, 1.0, 2.0, 3.0]))
    c = {"crossattn": torch.ones(6, 1, 4), "vector": torch.ones(6, 3), "concat": torch.ones(6, 4, 2, 2)}
    uc = {k: torch.zeros_like(v) for k, v in c.items()}
    x2, s2, cc = gd.prepare_inputs(x_u, torch.ones(6), c, uc)
    assert x2.shape[0] == 12 and s2.shape[0] == 12 and all(cc[k].shape[0] == 12 and not cc[k][:6].any() and cc[k][6:].all() for k in c)
    assert gd.prepare_inputs(x_u, torch.ones(6), c, uc)[2] is cc  # built once per (c, uc) pair


def test_svd_yaml_instantiates_hip_class():
    import yaml
    from cremage_amd.ldm_hip.latent_diffusion import instantiate_from_config
    from cremage_amd.pipeline import SVD_XT_UNET
    from cremage_amd.sgm_hip.video import SpatialVideoTransformer, VideoResBlock, VideoUNet
    p = yaml.safe_load(open(ROOT / "cremage_amd" / "configs" / "svd_xt-hip.yaml"))["model"]["params"]
    assert p["network_config"]["target"] == "cremage_amd.sgm_hip.video.VideoUNet"
    assert p["denoiser_config"]["params"]["scaling_config"]["target"].endswith("VScalingWithEDMcNoise")
    assert p["first_stage_config"]["params"]["decoder_config"]["target"].endswith("temporal_ae.VideoDecoder")  # stays the reference's
    assert p["network_config"]["params"] == SVD_XT_UNET
    u = dict(p["network_config"]["params"], model_channels=32, num_head_channels=16, context_dim=64, adm_in_channels=48)  # shrink
    unet = instantiate_from_config({"target": p["network_config"]["target"], "params": u})
    assert isinstance(unet, VideoUNet)
    assert isinstance(unet.middle_block[0], VideoResBlock) and isinstance(unet.middle_block[1], SpatialVideoTransformer)
    assert tuple(unet.middle_block[0].time_stack.in_layers[2].weight.shape) == (128, 128, 3, 1, 1)
    assert tuple(unet.input_blocks[0][0].weight.shape) == (32, 8, 3, 3)


def test_video_abi_is_declared_and_bound():
    """additive C ABI: the four entry points are declared in the header, bound in _lib.SIGNATURES, and the version stays 104"""
    header = (ROOT / "include" / "crg_hip.h").read_text()
    lib = (ROOT / "cremage_amd" / "_lib.py").read_text()
    for name in ("crg_conv_frames", "crg_attention_frames", "crg_add_frames", "crg_lincomb_frames"):
        assert re.search(rf"\bint {name}\(", header), name
        assert f'"{name}"' in lib, name
    assert "video.hip" in (ROOT / "cremage_amd" / "build.py").read_text()
    assert re.search(r"#define CRG_VERSION 104\b", (ROOT / "cremage_amd" / "csrc" / "crg_api.hip").read_text() + header)
