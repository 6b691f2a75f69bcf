#!/usr/bin/env python
"""SDXL refiner cost at 1024x1024 (128x128 latents, bf16 UNets, fp32 latents), eager, warmed up, device-synchronised.

Prints one JSON line:
  unet_ms_base_b2                  one base UNet call, CFG-doubled batch of one image (B = 2)
  unet_ms_refiner_b2 / _b4         one refiner UNet call at B = 2 and B = 4
  dpmpp2m30_ms_base                30 DPM++ 2M steps of the base alone (txt2img_sdxl, no decode)
  dpmpp2m30_ms_refined             the same run with the refiner at strength 0.15: 27 base + 3 refiner calls (txt2img_sdxl_refined)
  sampler_step_ms_{fused,unfused}  per-step sampler work outside the UNet: the DPM++ 2M loop with a network that returns a fixed
                                   eps, fused (input build + crg_cfg_dpmpp2m_step) against the unfused torch path
`--trace N` runs only the fused loop with the fixed-eps network for N steps (a profiler run:
rocprofv3 --kernel-trace --stats -- python tools/refiner_time.py --trace 5): every kernel it launches is sampler-side."""
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cremage_amd import pipeline as P  # noqa: E402
from cremage_amd.sgm_hip.sampling import DiscreteDenoiser, DPMPP2MSampler, VanillaCFG  # noqa: E402
from cremage_amd.synth import synth_input  # noqa: E402


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


def cond(tag, b, cdim, vdim, dev):
    return ({"crossattn": synth_input(tag + ".c", (b, 77, cdim), 1).to(dev), "vector": synth_input(tag + ".cv", (b, vdim), 1).to(dev)},
            {"crossattn": synth_input(tag + ".uc", (b, 77, cdim), 1).to(dev), "vector": synth_input(tag + ".ucv", (b, vdim), 1).to(dev)})


def sampler_only(steps, fused, dev, L):
    """The DPM++ 2M loop around a network that returns one fixed eps tensor (no UNet work): the sampler-side cost per run."""
    eps = synth_input("rt.eps", (2, 4, L, L), 3).to(dev)
    net = lambda x, t, c: eps  # noqa: E731
    den = DiscreteDenoiser().to(dev)
    c, uc = {"vector": torch.ones(1, 8, device=dev)}, {"vector": torch.zeros(1, 8, device=dev)}
    x0 = synth_input("rt.x0", (1, 4, L, L), 4).to(dev)
    smp = DPMPP2MSampler(steps, VanillaCFG(5.0), device=dev, fused=fused)
    return lambda: smp(lambda inp, sigma, cc: den(net, inp, sigma, cc), x0, cond=c, uc=uc, parts=(den, net))


def main():
    dev = torch.device("cuda:0")
    L = 128
    if "--trace" in sys.argv:
        n = int(sys.argv[sys.argv.index("--trace") + 1])
        with torch.no_grad():
            sampler_only(n, True, dev, L)()
        torch.cuda.synchronize()
        print(json.dumps(dict(trace_steps=n)), flush=True)
        return
    base = P.build_synthetic_sdxl(device=dev, seed=1)
    ref = P.build_synthetic_sdxl_refiner(device=dev, seed=2, first_stage=base.first_stage_model)
    c, uc = cond("rt.base", 1, 2048, 2816, dev)
    c2, uc2 = cond("rt.ref", 1, 1280, 2560, dev)
    x0 = synth_input("rt.x", (1, 4, L, L), 5).to(dev)
    out = dict(hw=8 * L, unet_dtype="bf16")
    with torch.no_grad():
        for tag, eng, cc, ucc, b in (("base_b2", base, c, uc, 1), ("refiner_b2", ref, c2, uc2, 1), ("refiner_b4", ref, c2, uc2, 2)):
            cat = {k: torch.cat([ucc[k]] * b + [cc[k]] * b) for k in cc}
            x = synth_input("rt.xx", (2 * b, 4, L, L), 6).to(dev)
            t = torch.full((2 * b,), 150, device=dev, dtype=torch.long)
            out["unet_ms_" + tag] = round(timed(lambda: eng.model(x, t, cat), 10), 3)
        out["dpmpp2m30_ms_base"] = round(timed(lambda: P.txt2img_sdxl(base, c, uc, steps=30, sampler="dpmpp2m", x0=x0, decode=False), 2), 1)
        out["dpmpp2m30_ms_refined"] = round(timed(lambda: P.txt2img_sdxl_refined(base, ref, c, uc, c2, uc2, steps=30, refiner_strength=0.15,
                                                                                  x0=x0, decode=False), 2), 1)
        for tag, fused in (("fused", True), ("unfused", False)):
            out["sampler_step_ms_" + tag] = round(timed(sampler_only(30, fused, dev, L), 5) / 30, 4)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
