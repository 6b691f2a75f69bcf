#!/usr/bin/env python
"""What the MX8 feed-forward (FeedForward(precision="mx8")) costs and buys, measured on the GPU.

default      device time of the feed-forward chain of one transformer block per UNet level, inside a captured hipGraph, the default arm
             and the MX8 arm alternating in one process.  The chain is what BasicTransformerBlock runs: the attention out-projection
             that PRODUCES the feed-forward's input (with the row statistics the default arm's LayerNorm epilogue wants; timed alone as
             well and subtracted), then norm3 + GEGLU projection + net[2] + residual.
               SD1.5 at 4 x 512^2 under CFG: M 32768 / 8192 / 2048 at C 320 / 640 / 1280;  SDXL at 1024^2: M 8192 / 2048 at C 640 / 1280.
--accuracy   rel-L2 of one UNet call against the fp32 golden of tests/golden, default feed-forward against MX8, for the small and the
             full-size SD1.5 and SDXL configurations (--no-full skips the full-size ones), and (--traj) latent / pixel error of the
             full-size 20-step SD1.5 trajectory as tests/test_hip_models.py::test_c1_sd15_full_20_step_trajectory states it.
One JSON line per figure."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import cremage_amd  # noqa: E402
from cremage_amd import ops  # noqa: E402

DEV = "cuda:0"
LEVELS = [("sd15", 32768, 320), ("sd15", 8192, 640), ("sd15", 2048, 1280), ("sdxl", 8192, 640), ("sdxl", 2048, 1280)]


def _graph(f, n):
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s), torch.no_grad():
        for _ in range(3):
            f()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.no_grad(), torch.cuda.graph(g):
        for _ in range(n):
            f()
    g.replay()
    torch.cuda.synchronize()
    return g


def _us(g, n, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        g.replay()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / (n * reps)


def timing(a):
    from cremage_amd.ldm_hip.transformer import FeedForward
    for model, M, C in LEVELS:
        torch.manual_seed(C)
        ff = FeedForward(C, glu=True).to(ops.HALF).to(DEV).eval()
        ln = torch.nn.LayerNorm(C).to(ops.HALF).to(DEV)
        src = torch.randn(M, C, device=DEV).to(ops.HALF)
        wo = (torch.randn(C, C, device=DEV) * C ** -0.5).to(ops.HALF)
        bo = torch.randn(C, device=DEV)
        stats = ops.ln_epi_wanted(C, geglu=True)

        def produce():
            return ops.linear(src, wo, bo, residual=src, row_stats=stats)

        def chain(precision):
            def f():
                ff.precision = precision
                x = produce()
                return ff(x, residual=x, ln=ln)
            return f
        n = max(2, min(20, (1 << 20) // M))
        reps = a.reps
        graphs = {"producer": _graph(produce, n), "default": _graph(chain(None), n), "mx8": _graph(chain("mx8"), n)}
        rounds = {k: [] for k in graphs}
        for _ in range(a.rounds):
            for k, g in graphs.items():
                rounds[k].append(_us(g, n, reps))
        med = {k: sorted(v)[len(v) // 2] for k, v in rounds.items()}
        flops = 2.0 * M * C * (8 * C + 4 * C)
        print(json.dumps({"figure": "ff_chain_us", "model": model, "M": M, "C": C, "default_us": round(med["default"] - med["producer"], 1),
                          "mx8_us": round(med["mx8"] - med["producer"], 1), "producer_us": round(med["producer"], 1),
                          "mx8_over_default": round((med["mx8"] - med["producer"]) / (med["default"] - med["producer"]), 3),
                          "default_tflops": round(flops / (med["default"] - med["producer"]) / 1e6, 1),
                          "mx8_tflops": round(flops / (med["mx8"] - med["producer"]) / 1e6, 1),
                          "rounds_us": {k: [round(t, 1) for t in v] for k, v in rounds.items()}}), flush=True)
        del graphs


def accuracy(a):
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from cremage_amd.synth import synth_fill_, synth_input
    from tests.conftest import GOLD, load_golden, rel_l2
    cases = [("unet_small_sd", False), ("sgm_unet_small_sdxl", True)]
    if not a.no_full:
        cases += [("unet_sd15_full", False), ("sgm_unet_sdxl_full", True)]
    for name, xl in cases:
        if not os.path.exists(os.path.join(GOLD, name + ".npz")):
            print(json.dumps({"figure": "unet_rel_l2", "case": name, "error": "golden not present"}), flush=True)
            continue
        meta, g = load_golden(name)
        cfg = meta["cfg"]
        if xl:
            from cremage_amd.sgm_hip.unet import UNetModel
        else:
            from cremage_amd.ldm_hip.unet import UNetModel
        m = synth_fill_(UNetModel(**cfg), meta["seed"], prefix=meta["prefix"]).to(ops.HALF).to(DEV).eval()
        B, L = tuple(g["y"].shape)[0], tuple(g["y"].shape)[-1]
        x = synth_input(name + ".x", (B, 4, L, L), meta["seed"]).to(DEV)
        ctx = synth_input(name + ".ctx", (B, meta.get("m", 77), cfg["context_dim"]), meta["seed"]).to(DEV)
        kw = dict(timesteps=g["t"].to(DEV), context=ctx)
        if xl:
            kw["y"] = synth_input(name + ".y", (B, cfg["adm_in_channels"]), meta["seed"]).to(DEV)
        res = {}
        with torch.no_grad():
            for prec in (None, "mx8"):
                n_ff = cremage_amd.set_ff_precision(m, prec)
                res[prec or "default"] = rel_l2(m(x, **kw).float().cpu(), g["y"])
        print(json.dumps({"figure": "unet_rel_l2", "case": name, "feed_forwards": n_ff, "default": res["default"], "mx8": res["mx8"]}), flush=True)
        del m
        torch.cuda.empty_cache()
    if a.traj:
        from cremage_amd import pipeline as P
        meta, g = load_golden("traj_c1_sd15_full")
        B, L, seed = meta["B"], meta["L"], meta["seed"]
        c = synth_input("c1.c", (B, 77, 768), seed).to(DEV)
        uc = synth_input("c1.uc", (B, 77, 768), seed).to(DEV)
        x0 = synth_input("c1.x0", (B, 4, L, L), seed).to(DEV)
        ref_pix = ((g["img_f16"].float() + 1) / 2).clamp(0, 1)
        for prec in (None, "mx8"):
            ldm = P.build_synthetic_ldm(meta["unet"], meta["dd"], DEV, unet_dtype=ops.HALF, vae_dtype=torch.float32, seed=seed)
            cremage_amd.set_ff_precision(ldm, prec)
            images, x = P.txt2img(ldm, c, uc, steps=meta["S"], sampler="euler", cfg_scale=meta["cfg"], height=8 * L, width=8 * L, x0=x0)
            pix = (images.cpu() - ref_pix).abs()
            print(json.dumps({"figure": "c1_trajectory", "feed_forward": prec or "default", "latent_rel_l2": rel_l2(x.float().cpu(), g["x"]),
                              "pixel_linf": pix.max().item(), "pixel_mean_abs": pix.mean().item()}), flush=True)
            del ldm
            torch.cuda.empty_cache()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--accuracy", action="store_true")
    ap.add_argument("--no-full", action="store_true")
    ap.add_argument("--traj", action="store_true")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=10)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("mx8_time.py measures on the GPU; no HIP device is visible")
    (accuracy if a.accuracy else timing)(a)
