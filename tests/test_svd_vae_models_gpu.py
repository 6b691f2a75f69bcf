"""The SVD first stage of cremage_amd.sgm_hip.video_vae on a real MI355X, against fixtures made by the reference's own VideoResBlock,
AE3DConv and VideoDecoder (tools/gen_golden_svd_vae.py).  Blocks at TOL_BLOCK, decoders in the fp32 class at TOL_NET[float32] plus the
pixel bound of tests/test_hip_models.py::test_vae_sd15_full_decode_pixels (L-inf < 1e-3 on clamp((x + 1) / 2, 0, 1); the fixtures
here hold the reference's fp32 output itself, so no allowance for an fp16-stored reference is added).

Half-type decoders have no project number to take: TOL_VAE_HALF is 1.5 x the rel-L2 measured on MI355X against the fp32 fixtures (the
rule DESIGN 6 f16 cites; figures in DESIGN 6 f17)."""
import pytest
import torch

from cremage_amd.synth import synth_fill_, synth_input
from tests.conftest import load_golden
from tests.test_hip_models import BF, DEV, TOL_BLOCK, TOL_NET, close, img, prep

pytestmark = pytest.mark.gpu

DTYPES = [torch.float32, BF]
# measured (bf16, MI355X): tiny decoder 9.35e-3 (skip_video 7.35e-3), full-width decoder 1.35e-2, chunked decode 9.85e-3; bounds = 1.5 x
TOL_VAE_HALF = {"svd_vae_dec_tiny": 1.40e-2, "svd_vae_dec_tiny skip": 1.10e-2, "svd_vae_dec_full": 2.02e-2, "svd_vae_chunked": 1.48e-2}


def _pixels(dec):
    return ((dec.detach().float().cpu() + 1) / 2).clamp(0, 1)


def _decoder(meta, dtype, cls=None, **kw):
    from cremage_amd.sgm_hip.video_vae import VideoDecoder
    m = (cls or VideoDecoder)(**meta["dd"], **({} if cls else dict(video_kernel_size=meta["video_kernel_size"])), **kw)
    return prep(m, meta, dtype)


def _latents(name, meta, dtype, frames=None):
    z = synth_input(name + ".z", (frames or meta["b"] * meta["t"], meta["dd"]["z_channels"], meta["hw"], meta["hw"]), meta["seed"])
    return img(z / meta["scale_factor"], dtype)


# -------------------------------------------------------------------------------------------------------------------------- blocks
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("strategy", ["learned", "fixed"])
@pytest.mark.parametrize("tag", ["svd_vae_res_skip", "svd_vae_res_same"])
def test_video_resblock(tag, strategy, dtype):
    from cremage_amd.sgm_hip.video_vae import VideoResBlock
    meta, g = load_golden(tag)
    m = prep(VideoResBlock(meta["cout"], in_channels=meta["cin"], temb_channels=0, dropout=0.0, video_kernel_size=[3, 1, 1],
                           alpha=meta["fixed_alpha"], merge_strategy=strategy), meta, dtype)
    assert ("mix_factor" in dict(m.named_buffers())) == (strategy == "fixed") and ("mix_factor" in dict(m.named_parameters())) == (strategy == "learned")
    assert abs(float(m.get_alpha().detach()) - meta["alpha_" + strategy]) < (1e-6 if dtype == torch.float32 else 4e-3)
    x = img(synth_input(tag + ".x", (meta["b"] * meta["t"], meta["cin"], meta["hw"], meta["hw"]), meta["seed"]), dtype)
    with torch.no_grad():
        y = m(x, None, timesteps=meta["t"])
    close(y, g["y_" + strategy], TOL_BLOCK[dtype], f"{tag} {strategy} {dtype}")


@pytest.mark.parametrize("dtype", DTYPES)
def test_ae3d_conv(dtype):
    from cremage_amd.sgm_hip.video_vae import AE3DConv
    tag = "svd_vae_ae3d"
    meta, g = load_golden(tag)
    m = prep(AE3DConv(meta["cin"], meta["cout"], video_kernel_size=[3, 1, 1], kernel_size=3, stride=1, padding=1), meta, dtype)
    x = img(synth_input(tag + ".x", (meta["b"] * meta["t"], meta["cin"], meta["hw"], meta["hw"]), meta["seed"]), dtype)
    with torch.no_grad():
        y, y_skip = m(x, meta["t"]), m(x, meta["t"], skip_video=True)
    close(y, g["y"], TOL_BLOCK[dtype], f"{tag} {dtype}")
    close(y_skip, g["y_skip"], TOL_BLOCK[dtype], f"{tag} skip_video {dtype}")


# ------------------------------------------------------------------------------------------------------------------------ decoders
def _check_decoder(dec, ref, dtype, what):
    if dtype == torch.float32:
        close(dec, ref, TOL_NET[torch.float32], what)
        linf = (_pixels(dec) - ((ref + 1) / 2).clamp(0, 1)).abs().max().item()
        print(f"\n[parity] {what}: pixel L-inf {linf:.3e}")
        assert linf < 1e-3, (what, linf)
    else:
        close(dec, ref, TOL_VAE_HALF[what.split(" [")[0]], what)


@pytest.mark.parametrize("dtype", DTYPES)
def test_video_decoder_tiny(dtype):
    name = "svd_vae_dec_tiny"
    meta, g = load_golden(name)
    m = _decoder(meta, dtype)
    z = _latents(name, meta, dtype)
    with torch.no_grad():
        dec = m(z, timesteps=meta["t"])
        dec_skip = m(z, timesteps=meta["t"], skip_video=True)
    assert dec.shape == (meta["b"] * meta["t"], 3, 2 * meta["hw"], 2 * meta["hw"])
    _check_decoder(dec, g["dec"], dtype, f"{name} [{dtype}]")
    _check_decoder(dec_skip, g["dec_skip"], dtype, f"{name} skip [{dtype}]")
    assert not torch.equal(dec, dec_skip)  # the temporal branch takes part


def test_video_decoder_full_width():
    """the YAML's decoder (ch 128, [1, 2, 4, 4], 2 res blocks): one video of 3 frames, 8 x 8 latents -> 64 x 64 pixels"""
    name = "svd_vae_dec_full"
    meta, g = load_golden(name)
    z32 = _latents(name, meta, torch.float32)
    for dtype in DTYPES:
        m = _decoder(meta, dtype)
        with torch.no_grad():
            dec = m(z32.to(dtype), timesteps=meta["t"])
        _check_decoder(dec, g["dec"], dtype, f"{name} [{dtype}]")
        del m


@pytest.mark.parametrize("dtype", DTYPES)
def test_skip_video_is_the_image_decoder(dtype):
    """skip_video=True runs the spatial layers only: bit for bit ldm_hip.vae.Decoder on the same spatial weights"""
    from cremage_amd.ldm_hip.vae import Decoder
    name = "svd_vae_dec_tiny"
    meta, _ = load_golden(name)
    mv = _decoder(meta, dtype)
    mi = _decoder(meta, dtype, cls=Decoder)  # the same names under the same prefix: the same spatial weights
    for k, v in mi.state_dict().items():
        assert torch.equal(v, mv.state_dict()[k]), k
    z = _latents(name, meta, dtype)
    with torch.no_grad():
        a, b = mv(z, timesteps=meta["t"], skip_video=True), mi(z)
    assert a.dtype == b.dtype and torch.equal(a, b)
    with torch.no_grad():  # and without `timesteps`, which the spatial path does not need
        assert torch.equal(mv(z, skip_video=True), b)


@pytest.mark.parametrize("dtype", DTYPES)
def test_only_last_conv_mode(dtype):
    """time_mode="only-last-conv": plain ResnetBlocks, the time mix behind the output conv only.  With skip_video the image Decoder bit
    for bit; without, conv_frames_thin on that Decoder's own output, bit for bit - and another function"""
    from cremage_amd import ops
    from cremage_amd.ldm_hip.vae import Decoder
    name = "svd_vae_dec_tiny"
    meta, _ = load_golden(name)
    mv = _decoder(meta, dtype, time_mode="only-last-conv")
    mi = _decoder(meta, dtype, cls=Decoder)
    assert not any(".time_stack." in k for k in mv.state_dict())
    z = _latents(name, meta, dtype)
    t = meta["t"]
    with torch.no_grad():
        img_dec = mi(z)
        assert torch.equal(mv(z, timesteps=t, skip_video=True), img_dec)
        mixed = mv(z, timesteps=t)
        tm = mv.conv_out.time_mix_conv
        want = ops.conv_frames_thin(ops.tokens_of(ops.to_channels_last(img_dec)), tm.weight, tm.bias, frames=t)
    assert mixed.shape == img_dec.shape and torch.isfinite(mixed).all() and not torch.equal(mixed, img_dec)
    assert torch.equal(ops.tokens_of(ops.to_channels_last(mixed)), want)


@pytest.mark.parametrize("dtype", DTYPES)
def test_bare_decode_is_one_video(dtype):
    """AutoencodingEngine.decode(z) without `timesteps` - how the reference's DiffusionEngine calls a decoder that is not its own class -
    decodes the batch as one video of len(z) frames: bit for bit decode(z, timesteps=len(z)), and not six one-frame videos"""
    from cremage_amd import pipeline as P
    name = "svd_vae_dec_tiny"
    meta, _ = load_golden(name)
    fs = P.build_synthetic_svd_vae(meta["dd"], device=DEV, vae_dtype=dtype, seed=meta["seed"])
    z = synth_input(name + ".z", (meta["b"] * meta["t"], 4, meta["hw"], meta["hw"]), meta["seed"]).to(DEV) / meta["scale_factor"]
    with torch.no_grad():
        bare, whole, single = fs.decode(z), fs.decode(z, timesteps=z.shape[0]), fs.decode(z, timesteps=1)
    assert torch.equal(bare, whole) and not torch.equal(bare, single)


def test_one_frame_is_the_centre_tap():
    """T = 1: both neighbours of the only frame of a video are padding, so the decoder equals the same call with the outer taps of every
    frame conv zeroed (the GroupNorms of the time stacks see one frame per video in both runs)"""
    name = "svd_vae_dec_tiny"
    meta, _ = load_golden(name)
    m = _decoder(meta, torch.float32)
    z = _latents(name, meta, torch.float32)
    with torch.no_grad():
        one = m(z, timesteps=1)
        taps = 0
        for k, p in m.named_parameters():
            if p.dim() == 5:
                p[:, :, 0].zero_()
                p[:, :, 2].zero_()
                taps += 1
        centre = m(z, timesteps=1)
        three = m(z, timesteps=meta["t"])
    assert taps == (meta["n_temporal_keys"] - 2) // 9 * 2 + 1  # two frame convs per VideoResBlock (9 temporal keys each) and time_mix_conv
    close(one, centre.float().cpu(), TOL_NET[torch.float32], "T = 1 vs centre tap")
    assert not torch.equal(three, centre)  # with three frames per video the time stacks normalise over them: another function


@pytest.mark.parametrize("dtype", DTYPES)
def test_decode_video_chunked(dtype):
    """pipeline.decode_video with decoding_t = 2 on 5 frames (chunks 2, 2, 1, each one video) through the AutoencodingEngine"""
    from cremage_amd import pipeline as P
    name = "svd_vae_chunked"
    meta, g = load_golden(name)
    fs = P.build_synthetic_svd_vae(meta["dd"], device=DEV, vae_dtype=dtype, seed=meta["seed"])
    z = synth_input(name + ".z", (meta["frames"], 4, meta["hw"], meta["hw"]), meta["seed"]).to(DEV)
    dec = P.decode_video(fs, z, meta["scale_factor"], decoding_t=meta["decoding_t"])
    assert dec.dtype == torch.float32 and dec.shape == g["dec"].shape
    _check_decoder(dec, g["dec"], dtype, f"{name} [{dtype}]")
    whole = P.decode_video(fs, z, meta["scale_factor"])
    assert not torch.equal(whole, dec)  # one video of 5 frames pads elsewhere: the chunking is the reference's behaviour, kept


def test_engine_encode_is_the_regularised_sample():
    from cremage_amd import pipeline as P
    meta, _ = load_golden("svd_vae_dec_tiny")
    fs = P.build_synthetic_svd_vae(meta["dd"], device=DEV, seed=meta["seed"])
    x = synth_input("svd_vae.img", (2, 3, 16, 16), meta["seed"], 0.5).clamp(-1, 1).to(DEV)
    noise = synth_input("svd_vae.noise", (2, 4, 8, 8), meta["seed"]).to(DEV)
    with torch.no_grad():
        moments, _ = fs.encode(x, unregularized=True)
        z = fs.encode(x, noise=noise)
    mean, logvar = moments.chunk(2, dim=1)
    assert torch.equal(z, mean + torch.exp(0.5 * logvar.clamp(-30.0, 20.0)) * noise) and z.shape == (2, 4, 8, 8)


def test_video_decoder_batch_invariant():
    """set_batch_invariant(): video 0 of two equals video 0 alone, bit for bit"""
    import cremage_amd
    name = "svd_vae_dec_tiny"
    meta, _ = load_golden(name)
    m = _decoder(meta, torch.float32)
    z = _latents(name, meta, torch.float32)
    t = meta["t"]
    cremage_amd.set_batch_invariant(8)
    try:
        with torch.no_grad():
            both = m(z, timesteps=t)
            solo = m(z[:t].contiguous(memory_format=torch.channels_last), timesteps=t)
    finally:
        cremage_amd.set_batch_invariant(0)
    assert torch.equal(both[:t], solo)
