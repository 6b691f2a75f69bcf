"""The modules that call `ops.attention` on fp32 tensors, with the fp32-class flash kernel switched on (ops.knobs.ATTN_X3_FLASH, what
CRG_ATTN_X3=1 sets): the goldens and bounds these fixtures carry in tests/test_hip_models.py, unchanged."""
import pytest
import torch

from cremage_amd.synth import synth_fill_, synth_input
from tests.conftest import load_golden
from tests.test_hip_models import DEV, TOL_BLOCK, TOL_NET, close, img, prep

pytestmark = pytest.mark.gpu
F32 = torch.float32


@pytest.fixture
def x3(monkeypatch):
    """knob on; counts the launches of the new kernel, so that a test cannot pass on the unfused branch"""
    from cremage_amd import _lib as L
    from cremage_amd import ops
    monkeypatch.setattr(ops.knobs, "ATTN_X3_FLASH", True)
    lib, calls = L.load(), []

    class Counting:
        def __getattr__(self, a):
            fn = getattr(lib, a)
            if a != "crg_attention_x3":
                return fn

            def rec(*args):
                calls.append(args[2]._obj.Dh)
                return fn(*args)
            return rec
    monkeypatch.setattr(L, "load", lambda: Counting())
    return calls


def test_vae_attn_block(x3):
    from cremage_amd.ldm_hip import vae as V
    meta, g = load_golden("blk_vae_attn")
    m = prep(V.AttnBlock(64), meta, F32)
    with torch.no_grad():
        close(m(img(synth_input("vattn.x", (2, 64, 6, 6), meta["seed"]), F32)), g["y"], TOL_BLOCK[F32], "vattn")
    assert x3 == [64]


@pytest.mark.parametrize("tag", ["ca_d40_m77", "ca_d80_m154", "ca_d160_self", "ca_d64_m77", "ca_d40_self"])
def test_cross_attention(x3, tag):
    from cremage_amd.ldm_hip.transformer import CrossAttention
    meta, g = load_golden("op_" + tag)
    m = prep(CrossAttention(meta["query_dim"], meta["context_dim"], heads=meta["heads"], dim_head=meta["dim_head"]), meta, F32)
    x = synth_input(tag + ".x", (2, meta["n"], meta["query_dim"]), meta["seed"]).to(DEV)
    ctx = synth_input(tag + ".ctx", (2, meta["m"], meta["context_dim"]), meta["seed"]).to(DEV) if meta["m"] else None
    with torch.no_grad():
        y = m(x, context=ctx)
        y_again = m(x, context=ctx)
    close(y, g["y"], TOL_BLOCK[F32], tag)
    assert torch.equal(y, y_again)
    assert x3 == [meta["dim_head"]] * 2


def test_cross_attention_lora_ipa(x3):
    """LoRA folded into the packed weights + the IP-Adapter FaceID second attention: both attentions take the flash route"""
    from cremage_amd.ldm_hip.transformer import CrossAttention
    meta, g = load_golden("op_ca_lora_ipa")
    tag = "ca_lora_ipa"
    m = CrossAttention(128, 96, heads=4, dim_head=32, lora_ranks=[4], lora_weights=[0.7], ipa_scale=0.6, ipa_num_tokens=4)
    synth_fill_(m, meta["seed"], prefix=meta["prefix"])
    with torch.no_grad():
        for name, p in m.named_parameters():
            if "_lora_" in name and p.ndim > 0:
                p.copy_(synth_input(tag + "." + name, p.shape, meta["seed"], 0.2))
    m = m.to(DEV).eval()
    x = synth_input(tag + ".x", (2, 50, 128), meta["seed"]).to(DEV)
    ctx = synth_input(tag + ".ctx", (2, 81, 96), meta["seed"]).to(DEV)
    with torch.no_grad():
        y = m(x, context=ctx)
    close(y, g["y"], TOL_BLOCK[F32], tag)
    assert x3 == [32, 32]


def test_vae_tiny(x3):
    from cremage_amd.ldm_hip.vae import AutoencoderKL
    meta, g = load_golden("vae_tiny")
    m = prep(AutoencoderKL(meta["dd"], None, 4), meta, F32)
    z = synth_input("vae_tiny.z", (2, 4, 8, 8), meta["seed"]).to(DEV)
    im = synth_input("vae_tiny.img", (2, 3, 16, 16), meta["seed"], 0.5).clamp(-1, 1).to(DEV)
    noise = synth_input("vae_tiny.noise", (2, 4, 8, 8), meta["seed"]).to(DEV)
    with torch.no_grad():
        close(m.decode(z), g["dec"], TOL_NET[F32], "vae dec")
        post = m.encode(im)
        close(post.parameters, g["moments"], TOL_NET[F32], "vae moments")
        close(post.sample(noise), g["sample"], TOL_NET[F32], "vae sample")
    assert len(x3) >= 2  # the mid-block attention of the decoder and of the encoder


def test_vae_sd15_full_decode_pixels(x3):
    """North-star bound with the AttnBlock (N 4096, d_head 512) on the flash kernel: L-inf on the exact fp32 subsample below 1e-3 in
    pixel units, as test_hip_models.test_vae_sd15_full_decode_pixels states it (knob off: 1.8e-5 .. 2.0e-5)."""
    from cremage_amd.ldm_hip.vae import AutoencoderKL
    meta, g = load_golden("vae_sd15_full_decode")
    m = prep(AutoencoderKL(meta["dd"], None, 4), meta, F32)
    z = synth_input("vae_full.z", (1, 4, 64, 64), meta["seed"]).to(DEV)
    with torch.no_grad():
        dec = m.decode(z / meta["scale_factor"]).cpu()
    assert dec.shape == (1, 3, 512, 512)
    sub = (dec[:, :, ::8, ::8] - g["dec_sub"]).abs().max().item()
    print(f"[fig] SD1.5 VAE decode, CRG_ATTN_X3: L-inf on the fp32 subsample {sub / 2:.3e} (pixel units, bound 1.000e-03)")
    assert sub / 2 < 1e-3
    assert x3 == [512]


def test_unet_tiny(x3):
    from cremage_amd.ldm_hip.unet import UNetModel
    meta, g = load_golden("unet_tiny")
    cfg = meta["cfg"]
    m = prep(UNetModel(**cfg), meta, F32)
    x = synth_input("unet_tiny.x", (meta["B"], 4, meta["L"], meta["L"]), meta["seed"]).to(DEV)
    ctx = synth_input("unet_tiny.ctx", (meta["B"], meta["m"], cfg["context_dim"]), meta["seed"]).to(DEV)
    with torch.no_grad():
        y = m(x, timesteps=g["t"].to(DEV), context=ctx)
    close(y, g["y"], TOL_NET[F32], "unet_tiny")
    assert x3
