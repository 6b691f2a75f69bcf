#!/usr/bin/env python
"""Cost of the SD1.5 k-diffusion samplers of cremage_amd.samplers.KSampler next to Euler A, on the flagship workload: 4 x 512x512
(64x64 latents), 20 steps, bf16 UNet, fp32 latents, CFG 7.5, eager, warmed up, device-synchronised, the sampler's default noise.

Prints one JSON line per sampler:
  run_ms_fused / run_ms_unfused   one sampling run (no decode) through the fused executor (one input build and one step launch per UNet
                                  evaluation) and through the torch executor; Euler A has its fused step only
  unet_calls                      UNet evaluations of that run
  outside_ms_per_call_*           sampler work outside the UNet per evaluation: the same run around a model whose apply_model returns
                                  a fixed eps
  rel_l2_fused_unfused            the fused run's latents against the unfused run's (same seed, same draws)
and a last line with one UNet call on the CFG-doubled batch (unet_ms_b8)."""
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cremage_amd import pipeline as P  # noqa: E402
from cremage_amd import samplers as K  # noqa: E402
from cremage_amd.synth import synth_input  # noqa: E402

STEPS, CFG, B, L = 20, 7.5, 4, 64


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


class FixedEps:
    """A LatentDiffusion-like model that does no work: the sampler and wrapper code around it is what is timed."""

    def __init__(self, ldm, eps):
        self.alphas_cumprod, self.num_timesteps, self.device, self.eps = ldm.alphas_cumprod, ldm.num_timesteps, ldm.device, eps

    def apply_model(self, x, t, cond):
        return self.eps


def make(model, key, fused):
    return P.SAMPLERS[key](model) if key == "euler_a" else P.SAMPLERS[key](model, fused=fused)


def run(smp, x0, c, uc, seed=0):
    torch.manual_seed(seed)
    return smp.sample(S=STEPS, conditioning=c, batch_size=B, shape=[4, L, L], verbose=False, unconditional_guidance_scale=CFG,
                      unconditional_conditioning=uc, x0=x0)[0]


def main():
    dev = torch.device("cuda:0")
    ldm = P.build_synthetic_ldm(device=dev, seed=1)
    c, uc = synth_input("kt.c", (B, 77, 768), 1).to(dev), synth_input("kt.uc", (B, 77, 768), 1).to(dev)
    x0 = synth_input("kt.x", (B, 4, L, L), 5).to(dev)
    fixed = FixedEps(ldm, synth_input("kt.eps", (2 * B, 4, L, L), 3).to(dev))
    calls = [0]
    real = ldm.apply_model

    def counting(*a, **k):
        calls[0] += 1
        return real(*a, **k)
    ldm.apply_model = counting
    with torch.no_grad():
        for key in ("euler_a",) + K.K_SAMPLER_KEYS:
            out = dict(sampler=key, steps=STEPS, batch=B, hw=8 * L, unet_dtype="bf16")
            modes = (("fused", None),) if key == "euler_a" else (("fused", None), ("unfused", False))
            lat = {}
            for tag, fused in modes:
                smp = make(ldm, key, fused)
                out[f"run_ms_{tag}"] = round(timed(lambda: run(smp, x0, c, uc), 2), 1)
                calls[0] = 0
                lat[tag] = run(smp, x0, c, uc)
                out["unet_calls"] = calls[0]
                s2 = make(fixed, key, fused)
                out[f"outside_ms_per_call_{tag}"] = round(timed(lambda: run(s2, x0, c, uc), 5) / out["unet_calls"], 4)
            if "unfused" in lat:
                out["rel_l2_fused_unfused"] = float((lat["fused"] - lat["unfused"]).norm() / lat["unfused"].norm())
            print(json.dumps(out), flush=True)
        x = synth_input("kt.xx", (2 * B, 4, L, L), 6).to(dev)
        t = torch.full((2 * B,), 500, device=dev, dtype=torch.long)
        ctx = torch.cat([uc, c])
        print(json.dumps(dict(unet_ms_b8=round(timed(lambda: real(x, t, {"c_crossattn": [ctx]}), 10), 3))), flush=True)


if __name__ == "__main__":
    main()
