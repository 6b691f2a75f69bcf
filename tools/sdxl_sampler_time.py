#!/usr/bin/env python
"""Cost of Cremage's six SDXL samplers on both schedules at 1024x1024 (128x128 latents, one image, bf16 UNet, fp32 latents, CFG 5),
eager, warmed up, device-synchronised.

Prints one JSON line per (sampler, schedule):
  loop_ms              a 30-step txt2img_sdxl sampling loop (no decode)
  unet_calls           UNet evaluations in that loop
  outside_ms_per_call  sampler work outside the UNet per evaluation: the same loop around a network that returns a fixed eps,
                       fused (input build + one step launch) and unfused (the torch loop); Euler EDM has no fused path
  rel_l2_fused_unfused the full-size fused loop's latents against the unfused loop's (same seed, same noise draws)
and a last line with one base UNet call (unet_ms_b2)."""
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cremage_amd import pipeline as P  # noqa: E402
from cremage_amd.sgm_hip import sampling as S  # noqa: E402
from cremage_amd.synth import synth_input  # noqa: E402

STEPS, CFG = 30, 5.0
DISC = {"legacy": "legacy_ddpm", "edm": "edm"}


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


def make(eng, key, disc, fused):
    smp = eng.make_sampler(key, STEPS, CFG, torch.device("cuda:0"), discretization=DISC[disc])
    if hasattr(smp, "fused"):
        smp.fused = fused
    return smp


def run(eng, smp, x0, c, uc, seed=0):
    torch.manual_seed(seed)
    return eng.run_sampler(smp, x0, c, uc)


class FixedEps(torch.nn.Module):
    def __init__(self, eps):
        super().__init__()
        self.eps = eps

    def forward(self, x, t, c):
        return self.eps


def main():
    dev = torch.device("cuda:0")
    L = 128
    eng = P.build_synthetic_sdxl(device=dev, seed=1)
    c = {"crossattn": synth_input("st.c", (1, 77, 2048), 1).to(dev), "vector": synth_input("st.cv", (1, 2816), 1).to(dev)}
    uc = {"crossattn": synth_input("st.uc", (1, 77, 2048), 1).to(dev), "vector": synth_input("st.ucv", (1, 2816), 1).to(dev)}
    x0 = synth_input("st.x", (1, 4, L, L), 5).to(dev)
    # the fixed-eps engine: the same denoiser / sampler code around a network that does no work
    eps = synth_input("st.eps", (2, 4, L, L), 3).to(dev)
    fixed = S.DiffusionEngine(torch.nn.Identity(), torch.nn.Identity())
    fixed.model = FixedEps(eps)
    fixed.denoiser = fixed.denoiser.to(dev)
    calls = [0]
    real_forward = eng.model.forward

    def counting(*a, **k):
        calls[0] += 1
        return real_forward(*a, **k)
    eng.model.forward = counting
    with torch.no_grad():
        for key in S.SGM_SAMPLERS:
            for disc in DISC:
                out = dict(sampler=key, schedule=disc, steps=STEPS, hw=8 * L, unet_dtype="bf16")
                smp = make(eng, key, disc, True)
                out["loop_ms"] = round(timed(lambda: run(eng, smp, x0, c, uc), 1), 1)
                calls[0] = 0
                xf = run(eng, smp, x0, c, uc)
                out["unet_calls"] = calls[0]
                xu = run(eng, make(eng, key, disc, False), x0, c, uc)
                out["rel_l2_fused_unfused"] = float((xf - xu).norm() / xu.norm())
                for tag, fused in (("fused", True), ("unfused", False)):
                    if tag == "fused" and not hasattr(smp, "fused"):
                        continue
                    s2 = make(fixed, key, disc, fused)
                    out[f"outside_ms_per_call_{tag}"] = round(timed(lambda: run(fixed, s2, x0, c, uc), 5) / out["unet_calls"], 4)
                print(json.dumps(out), flush=True)
        x = synth_input("st.xx", (2, 4, L, L), 6).to(dev)
        t = torch.full((2,), 500, device=dev, dtype=torch.long)
        cat = {k: torch.cat([uc[k], c[k]]) for k in c}
        print(json.dumps(dict(unet_ms_b2=round(timed(lambda: real_forward(x, t, cat), 10), 3))), flush=True)


if __name__ == "__main__":
    main()
