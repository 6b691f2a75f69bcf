#!/usr/bin/env python
"""Inpainting cost against txt2img at the same shape: one batch of four 512x512 images (CFG-doubled UNet batch 8, 64x64 latents,
bf16 UNet, fp32 VAE), 20 DDIM steps at eta = 1 (inpaint.py's sampler), UNet calls replayed from captured hipGraphs.

Prints one JSON line:
  unet_ms_{txt2img,inpaint}   one graph-replayed UNet call: the 4-channel model vs the 9-channel model with c_concat folded into the
                              input conversion (both CFG-shared)
  ddim20_ms_{txt2img,inpaint} the 20-step DDIM loop (sampler + fused step), no encode / decode
  step_overhead_ms_*          loop time / 20 - one UNet call: the non-UNet work of a step
`--short` runs 5 steps and few repeats (a profiler run: rocprofv3 --kernel-trace --stats -- python tools/inpaint_time.py --short)."""
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cremage_amd import ops  # noqa: E402
from cremage_amd import pipeline as P  # noqa: E402
from cremage_amd.samplers import DDIMSampler  # noqa: E402
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


def main():
    short = "--short" in sys.argv
    steps, reps_call, reps_loop = (5, 3, 1) if short else (20, 30, 3)
    dev = torch.device("cuda:0")
    b, L = 4, 64
    txt = P.build_synthetic_ldm(device=dev, seed=1)
    inp = P.build_synthetic_inpaint_ldm(device=dev, seed=1)
    for m in (txt, inp):
        m.model.enable_hip_graph()
    c = synth_input("it.c", (b, 77, 768), 1).to(dev)
    uc = synth_input("it.uc", (b, 77, 768), 2).to(dev)
    cc = torch.cat([(synth_input("it.mask", (b, 1, L, L), 3) > 0).float(), synth_input("it.zm", (b, 4, L, L), 4)], 1).to(dev)
    x_T = synth_input("it.x", (b, 4, L, L), 5).to(dev)
    noise = synth_input("it.noise", (steps, b, 4, L, L), 6).to(dev)
    ctx2 = torch.cat([uc, c])
    cc2 = ops.mark_cfg_dup(torch.cat([cc, cc]))
    t2 = torch.full((2 * b,), 501, device=dev, dtype=torch.long)
    x2 = torch.cat([x_T, x_T])
    with torch.no_grad():
        unet_txt = timed(lambda: txt.apply_model(ops.mark_cfg_dup(x2.clone()), t2, {"c_crossattn": [ctx2]}), reps_call)
        unet_inp = timed(lambda: inp.apply_model(ops.mark_cfg_dup(x2.clone()), t2, {"c_concat": [cc2], "c_crossattn": [ctx2]}), reps_call)

        def loop(ldm, cond, ucond):
            it = iter(range(steps))
            DDIMSampler(ldm).sample(steps, b, [4, L, L], cond, eta=1.0, x_T=x_T, unconditional_guidance_scale=7.5,
                                    unconditional_conditioning=ucond, noise_sampler=lambda s, i: noise[next(it)])
        ddim_txt = timed(lambda: loop(txt, c, uc), reps_loop)
        ddim_inp = timed(lambda: loop(inp, {"c_concat": [cc], "c_crossattn": [c]}, {"c_concat": [cc], "c_crossattn": [uc]}), reps_loop)
    out = dict(batch=b, hw=8 * L, steps=steps, unet_ms_txt2img=round(unet_txt, 3), unet_ms_inpaint=round(unet_inp, 3),
               unet_ratio=round(unet_inp / unet_txt, 4), ddim_ms_txt2img=round(ddim_txt, 2), ddim_ms_inpaint=round(ddim_inp, 2),
               step_overhead_ms_txt2img=round(ddim_txt / steps - unet_txt, 3), step_overhead_ms_inpaint=round(ddim_inp / steps - unet_inp, 3),
               captures=[txt.model.graphed.captures, inp.model.graphed.captures])
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
