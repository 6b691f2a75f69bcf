"""Timings of the video path at SVD-XT's shapes (b = 2 for CFG, T = 25 frames, 72 x 128 latents; C = 320 / 640 / 1280 at 9216 / 2304 / 576
pixels per frame), each candidate captured into a hipGraph and replayed, median of the replays, random data:

  * ops.conv_frames against the composed route (per video three row-shifted GEMMs chained through their residual input) and against
    the project's 3x3 conv at equal pixels and channels (which does three times the multiplies);
  * ops.attention_frames against rearrange + the existing flash attention ((b t) s c -> (b s) t c copies of q, k, v and back);
  * one full-size VideoUNet call (svd_xt-hip.yaml's network, random weights) with its device-time share per kernel family.

    python tools/svd_time.py [--skip-unet] [--reps 20]
Prints one JSON line per measurement."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from cremage_amd import ops  # noqa: E402

DEV = "cuda:0"
B, T, H, W = 2, 25, 72, 128


def graph_ms(fn, reps):
    """median milliseconds of `fn` replayed from a captured graph"""
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.no_grad(), torch.cuda.graph(g):
        fn()
    g.replay()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        g.replay()
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1))
    return statistics.median(times), min(times)


def rnd(*shape, scale=1.0):
    return (torch.randn(*shape, device=DEV) * scale).to(ops.HALF)


def out(**kw):
    print(json.dumps(kw), flush=True)


def conv_rows(reps):
    for level, C in enumerate((320, 640, 1280)):
        h, w = H >> level, W >> level
        S, F = h * w, B * T
        x = rnd(F, S, C)
        wt = torch.randn(C, C, 3, 1, 1, device=DEV) * (3 * C) ** -0.5
        bias = torch.randn(C, device=DEV)
        taps = [wt[:, :, d, 0, 0].contiguous().to(ops.HALF) for d in range(3)]
        w33 = torch.randn(C, C, 3, 3, device=DEV) * (9 * C) ** -0.5
        ximg = ops.image_of(x, h, w)

        def composed():
            ys = []
            for v in range(B):
                xv = x[v * T:(v + 1) * T]
                y = ops.linear(xv, taps[1], bias)
                top = ops.linear(xv[:-1], taps[0], residual=y[1:])    # frames 1 .. T-1 take their predecessor
                y2 = torch.cat([y[:1], top])
                bot = ops.linear(xv[1:], taps[2], residual=y2[:-1])   # frames 0 .. T-2 take their successor
                ys.append((bot, y2[-1:]))
            return ys
        a = graph_ms(lambda: ops.conv_frames(x, wt, bias, frames=T), reps)
        c = graph_ms(composed, reps)
        k = graph_ms(lambda: ops.conv2d(ximg, w33, bias), reps)
        flops = 2.0 * F * S * C * 3 * C
        out(what="conv_frames", C=C, pixels=S, frames=F, ms=a[0], ms_min=a[1], tflops=flops / a[0] * 1e-9, composed_ms=c[0], conv3x3_ms=k[0])


def attention_rows(reps):
    for level, C in enumerate((320, 640, 1280)):
        h, w = H >> level, W >> level
        S, F, heads = h * w, B * T, C // 64
        qkv = rnd(F, S, 3 * C)
        q, k, v = qkv[..., :C], qkv[..., C:2 * C], qkv[..., 2 * C:]

        def rearranged():
            sw = lambda t: t.reshape(B, T, S, C).permute(0, 2, 1, 3).reshape(B * S, T, C).contiguous()
            o = ops.attention_rows_v(sw(q), sw(k), sw(v), heads, 64 ** -0.5)
            return o.reshape(B, S, T, C).permute(0, 2, 1, 3).reshape(F, S, C).contiguous()
        a = graph_ms(lambda: ops.attention_frames(q, k, v, heads, frames=T), reps)
        r = graph_ms(rearranged, reps)
        gb = 4.0 * F * S * C * 2 * 1e-9
        out(what="attention_frames", C=C, pixels=S, frames=F, heads=heads, ms=a[0], ms_min=a[1], tb_per_s=gb / a[0], rearranged_flash_ms=r[0])


def unet_row(reps):
    from cremage_amd.graphs import GraphedModule
    from cremage_amd.pipeline import SVD_XT_UNET
    from cremage_amd.sgm_hip.video import VideoUNet
    with torch.device("meta"):
        m = VideoUNet(**SVD_XT_UNET)
    m = m.to_empty(device=DEV)
    g = torch.Generator(device=DEV).manual_seed(0)
    with torch.no_grad():
        for name, p in m.named_parameters():
            if p.dim() > 1:
                p.copy_(torch.randn(p.shape, device=DEV, generator=g) * (p[0].numel() ** -0.5))
            else:
                p.copy_(torch.ones_like(p) if name.endswith("weight") else torch.zeros_like(p))
    m = m.to(ops.HALF).eval()
    F = B * T
    x = torch.randn(F, 8, H, W, device=DEV)
    ctx = torch.randn(F, 1, 1024, device=DEV)
    y = torch.randn(F, 768, device=DEV)
    t = torch.full((F,), 0.5, device=DEV)
    ind = torch.zeros(B, T, device=DEV)
    kw = dict(timesteps=t, context=ctx, y=y, num_video_frames=T, image_only_indicator=ind)
    gm = GraphedModule(m, scratch_bytes=1 << 30)
    with torch.no_grad():
        gm(x, **kw)
        times = []
        for _ in range(max(3, reps // 4)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            gm(x, **kw)
            e1.record()
            e1.synchronize()
            times.append(e0.elapsed_time(e1))
        with ops.profile() as prof:
            m(x, **kw)
    total = sum(f["ms"] for f in prof.result.values())
    out(what="video_unet_call", frames=F, latent=[H, W], params=sum(p.numel() for p in m.parameters()), ms=statistics.median(times), ms_min=min(times),
        kernel_ms=total, share={k: round(f["ms"] / total, 4) for k, f in sorted(prof.result.items(), key=lambda kv: -kv[1]["ms"]) if f["ms"] > 0})


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--skip-unet", action="store_true")
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    conv_rows(a.reps)
    attention_rows(a.reps)
    if not a.skip_unet:
        unet_row(a.reps)
