"""Timings of the SVD first stage's frame convs at the VideoDecoder's shapes for a 576 x 1024 video (72 x 128 latents; C = 512 at 9216 and
36864 pixels per frame, 256 at 147456, 128 at 589824), T = 8 and 14 frames, one video; each candidate captured into a hipGraph and
replayed, median of the replays, random data (the protocol of tools/svd_time.py):

  * ops.conv_frames_x3 (one launch on pre-split planes) against the composed fp32 arm of ops.conv_frames (per video three row-shifted
    fp32-class GEMMs and axpby passes over fp32 tensors) and against the fp32-class 3x3 conv on the same planes (three times the multiplies);
  * ops.conv_frames_thin on the 3 pixel channels;
  * one full VideoDecoder call (svd_xt_vae-hip.yaml's decoder, random weights, fp32 class) on 14 frames of 72 x 128 latents, with its
    device time per kernel family.

    python tools/svd_vae_time.py [--skip-decoder] [--reps 20] [--frames 8 14]
Prints one JSON line per measurement."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from cremage_amd import ops  # noqa: E402
from tools.svd_time import graph_ms  # noqa: E402

DEV = "cuda:0"
H, W = 72, 128
LEVELS = [(512, 1), (512, 2), (256, 4), (128, 8)]  # (channels, upsampling factor over the latent grid)


def out(**kw):
    print(json.dumps(kw), flush=True)


def conv_rows(reps, frames):
    for C, up in LEVELS:
        h, w = H * up, W * up
        S = h * w
        wt = torch.randn(C, C, 3, 1, 1, device=DEV) * (3 * C) ** -0.5
        w33 = torch.randn(C, C, 3, 3, device=DEV) * (9 * C) ** -0.5
        bias = torch.randn(C, device=DEV)
        for T in frames:
            x = torch.randn(T, S, C, device=DEV)
            hi_img, lo_img = ops.split_bf16(ops.image_of(x, h, w))
            hi, lo = ops.tokens_of(hi_img), ops.tokens_of(lo_img)
            a = graph_ms(lambda: ops.conv_frames_x3(hi, lo, wt, bias, frames=T), reps)
            c = graph_ms(lambda: ops.conv_frames(x, wt, bias, frames=T), reps)
            k = graph_ms(lambda: ops.conv2d(hi_img, w33, bias, x_lo=lo_img), reps)
            flops = 2.0 * T * S * C * 3 * C  # the conv's own multiplies; the kernel runs three matrix passes of them
            out(what="conv_frames_x3", C=C, pixels=S, frames=T, ms=a[0], ms_min=a[1], tflops=flops / a[0] * 1e-9, mfma_tflops=3 * flops / a[0] * 1e-9,
                composed_ms=c[0], speedup=c[0] / a[0], conv3x3_x3_ms=k[0])
            del x, hi_img, lo_img, hi, lo
            torch.cuda.empty_cache()


def thin_rows(reps, frames):
    S = H * 8 * W * 8
    wt = torch.randn(3, 3, 3, 1, 1, device=DEV) * 9 ** -0.5
    bias = torch.randn(3, device=DEV)
    for T in frames:
        for dtype in (torch.float32, ops.HALF):
            x = torch.randn(T, S, 3, device=DEV).to(dtype)
            a = graph_ms(lambda: ops.conv_frames_thin(x, wt, bias, frames=T), reps)
            gb = 2.0 * T * S * 3 * x.element_size() * 1e-9  # one read and one write of the tensor (the neighbour frames hit in cache or not)
            out(what="conv_frames_thin", C=3, pixels=S, frames=T, dtype=str(dtype), ms=a[0], ms_min=a[1], tb_per_s=gb / a[0])


def decoder_row(reps, T=14):
    from cremage_amd.pipeline import SVD_VAE_DD
    from cremage_amd.sgm_hip.video_vae import VideoDecoder
    with torch.device("meta"):
        m = VideoDecoder(**SVD_VAE_DD, video_kernel_size=[3, 1, 1])
    m = m.to_empty(device=DEV)
    g = torch.Generator(device=DEV).manual_seed(0)
    with torch.no_grad():
        for name, p in m.named_parameters():
            if p.dim() > 1:
                p.copy_(torch.randn(p.shape, device=DEV, generator=g) * (p[0].numel() ** -0.5))
            elif name.endswith("mix_factor"):
                p.fill_(0.0)  # sigmoid -> alpha 0.5
            else:
                p.copy_(torch.ones_like(p) if name.endswith("weight") else torch.zeros_like(p))
    m = m.eval()
    z = torch.randn(T, 4, H, W, device=DEV).contiguous(memory_format=torch.channels_last)
    with torch.no_grad():
        for skip in (False, True):
            m(z, timesteps=T, skip_video=skip)
            torch.cuda.synchronize()
            times = []
            for _ in range(max(3, reps // 6)):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                m(z, timesteps=T, skip_video=skip)
                e1.record()
                e1.synchronize()
                times.append(e0.elapsed_time(e1))
            with ops.profile() as prof:
                m(z, timesteps=T, skip_video=skip)
            total = sum(f["ms"] for f in prof.result.values())
            out(what="video_decoder_call", skip_video=skip, frames=T, latent=[H, W], params=sum(p.numel() for p in m.parameters()),
                ms=statistics.median(times), ms_min=min(times), kernel_ms=total,
                family_ms={k: round(f["ms"], 2) for k, f in sorted(prof.result.items(), key=lambda kv: -kv[1]["ms"]) if f["ms"] > 0},
                slot_ms={k: round(v["ms"], 2) for k, v in sorted(prof.kernels.items(), key=lambda kv: -kv[1]["ms"]) if v["ms"] > 0})


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--skip-decoder", action="store_true")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--frames", type=int, nargs="*", default=[8, 14])
    a = ap.parse_args()
    conv_rows(a.reps, a.frames)
    thin_rows(a.reps, a.frames)
    if not a.skip_decoder:
        decoder_row(a.reps)
