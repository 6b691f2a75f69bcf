"""ORACLE tooling for the SVD first stage - writes tests/golden/svd_vae_*.npz from the reference's own modules (sgm temporal_ae
VideoResBlock, AE3DConv and VideoDecoder at the svd_xt_1_1.yaml settings, decoded the way DiffusionEngine.decode_first_stage does), on
the name-keyed synthetic weights and `synth_input` tensors of oracle/gen_golden.py, whose import stubs and helpers it reuses (that module
is imported, not changed).  The fill re-randomises the zero-initialised second conv of every time_stack and draws the `learned`
mix_factor like any parameter; a `fixed` mix_factor is a buffer and keeps the alpha it is built with (0.3 here: 0 would switch the
temporal branch off).  Only outputs and metadata are stored; a rerun reproduces them exactly (apart from timing meta).

    python tools/gen_golden_svd_vae.py [--only NAME ...]
"""
import argparse
import hashlib
import math
import os
import sys
import time
import types

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from oracle import gen_golden as G  # noqa: E402  (installs the import stubs and puts the reference on sys.path)
from oracle.gen_golden import SEED, fp32_forward, save, synth_fill_, synth_input  # noqa: E402

# svd_xt_1_1.yaml first_stage_config.decoder_config
SVD_VAE_DD = dict(attn_type="vanilla", double_z=True, z_channels=4, resolution=256, in_channels=3, out_ch=3, ch=128, ch_mult=[1, 2, 4, 4],
                  num_res_blocks=2, attn_resolutions=[], dropout=0.0)
TINY_VAE_DD = dict(SVD_VAE_DD, resolution=64, ch=64, ch_mult=[1, 2], num_res_blocks=1)
KS = [3, 1, 1]
FIXED_ALPHA = 0.3
SCALE = 0.18215


def _modules():
    G._import_sgm()
    name = "sgm.modules.autoencoding"
    if name not in sys.modules:  # a bare package, like the ones oracle.gen_golden registers: its __init__ is not needed
        m = types.ModuleType(name)
        m.__path__ = [os.path.join(os.path.dirname(sys.modules["sgm.modules"].__path__[0]), "modules", "autoencoding")]
        sys.modules[name] = m
    from sgm.modules.autoencoding import temporal_ae
    from sgm.modules.diffusionmodules import model
    return temporal_ae, model


def _key_digest(module):
    items = sorted(f"{k}:{tuple(v.shape)}" for k, v in module.state_dict().items())
    return hashlib.sha1("\n".join(items).encode()).hexdigest(), len(items)


def _pix_stats(dec):
    img = torch.clamp((dec + 1.0) / 2.0, 0.0, 1.0)
    return torch.tensor([img.mean().item(), img.std().item(), dec.abs().max().item()])


def g_resblock():
    TA, _ = _modules()
    b, t, hw = 2, 3, 8
    for tag, cin, cout in [("svd_vae_res_skip", 128, 256), ("svd_vae_res_same", 128, 128)]:
        x = synth_input(tag + ".x", (b * t, cin, hw, hw), SEED)
        outs, meta = {}, {}
        for strategy in ("learned", "fixed"):
            m = TA.VideoResBlock(cout, in_channels=cin, temb_channels=0, dropout=0.0, video_kernel_size=KS, alpha=FIXED_ALPHA,
                                 merge_strategy=strategy)
            synth_fill_(m, SEED, prefix=tag + ".")
            with fp32_forward():
                outs["y_" + strategy] = m(x, None, timesteps=t)
            sha, n = _key_digest(m)
            meta.update({"n_keys_" + strategy: n, "keys_sha1_" + strategy: sha, "alpha_" + strategy: float(m.get_alpha(b).detach())})
        save(tag, dict(cin=cin, cout=cout, b=b, t=t, hw=hw, seed=SEED, prefix=tag + ".", fixed_alpha=FIXED_ALPHA, **meta), **outs)


def g_ae3d():
    TA, _ = _modules()
    tag, b, t, hw, cin, cout = "svd_vae_ae3d", 2, 3, 8, 128, 3
    m = TA.AE3DConv(cin, cout, video_kernel_size=KS, kernel_size=3, stride=1, padding=1)
    synth_fill_(m, SEED, prefix=tag + ".")
    x = synth_input(tag + ".x", (b * t, cin, hw, hw), SEED)
    with fp32_forward():
        y, y_skip = m(x, t), m(x, t, skip_video=True)
    sha, n = _key_digest(m)
    save(tag, dict(cin=cin, cout=cout, b=b, t=t, hw=hw, seed=SEED, prefix=tag + ".", n_keys=n, keys_sha1=sha), y=y, y_skip=y_skip)


def _decoder(dd):
    TA, _ = _modules()
    m = TA.VideoDecoder(**dd, video_kernel_size=KS)
    synth_fill_(m, SEED, prefix="svd_vae.decoder.")
    return m.eval()


def _engine_digest(dd, dec):
    """key layout of AutoencodingEngine (sgm/models/autoencoder.py:132-137): encoder.*, decoder.* - the loss (torch.nn.Identity) and the
    DiagonalGaussianRegularizer hold no tensors (the class itself is a LightningModule, which is not importable here)"""
    _, SV = _modules()
    box = torch.nn.Module()
    box.encoder, box.decoder = SV.Encoder(**dd), dec
    return _key_digest(box)


def _decoder_case(name, dd, b, t, hw, skip):
    m = _decoder(dd)
    z = synth_input(name + ".z", (b * t, dd["z_channels"], hw, hw), SEED)
    outs, t0 = {}, time.time()
    with fp32_forward():
        outs["dec"] = m(z / SCALE, timesteps=t)
        if skip:
            outs["dec_skip"] = m(z / SCALE, timesteps=t, skip_video=True)
    sha, n = _key_digest(m)
    esha, en = _engine_digest(dd, m)
    n_t = sum(1 for k in m.state_dict() if ".time_stack." in k or "mix_factor" in k or "time_mix_conv" in k)
    save(name, dict(dd=dd, video_kernel_size=KS, b=b, t=t, hw=hw, seed=SEED, prefix="svd_vae.decoder.", engine_prefix="svd_vae.",
                    scale_factor=SCALE, n_params=sum(p.numel() for p in m.parameters()), n_keys=n, keys_sha1=sha, n_temporal_keys=n_t,
                    engine_n_keys=en, engine_keys_sha1=esha, ref_cpu_seconds=time.time() - t0, threads=torch.get_num_threads()),
         pix_stats=_pix_stats(outs["dec"]), **outs)


def g_dec_tiny():
    _decoder_case("svd_vae_dec_tiny", TINY_VAE_DD, 2, 3, 8, True)


def g_dec_full():
    _decoder_case("svd_vae_dec_full", SVD_VAE_DD, 1, 3, 8, False)


def g_chunked():
    """DiffusionEngine.decode_first_stage (sgm/models/diffusion.py:118-136) with en_and_decode_n_samples_a_time = 2 on 5 frames:
    chunks of 2, 2 and 1 frames, each decoded as one video of len(chunk) frames"""
    name, frames, decoding_t, hw = "svd_vae_chunked", 5, 2, 8
    m = _decoder(TINY_VAE_DD)
    z = synth_input(name + ".z", (frames, 4, hw, hw), SEED)
    zz = 1.0 / SCALE * z
    out, lens = [], []
    with fp32_forward():
        for n in range(math.ceil(frames / decoding_t)):
            chunk = zz[n * decoding_t:(n + 1) * decoding_t]
            lens.append(len(chunk))
            out.append(m(chunk, timesteps=len(chunk)))
    out = torch.cat(out, dim=0)
    save(name, dict(dd=TINY_VAE_DD, video_kernel_size=KS, frames=frames, decoding_t=decoding_t, hw=hw, seed=SEED, prefix="svd_vae.decoder.",
                    engine_prefix="svd_vae.", scale_factor=SCALE, chunks=lens), dec=out, pix_stats=_pix_stats(out))


ALL = dict(resblock=g_resblock, ae3d=g_ae3d, dec_tiny=g_dec_tiny, dec_full=g_dec_full, chunked=g_chunked)

if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", nargs="*", default=None)
    a = ap.parse_args()
    torch.manual_seed(0)
    for key, fn in ALL.items():
        if a.only and key not in a.only:
            continue
        fn()
