#!/usr/bin/env python
"""bench.py - images/sec of the SD1.5 denoising path on MI355X (BASELINE.json metric).

Workload (BASELINE.json configs[1], "C2"): SD1.5 txt2img 512x512, batch 4 per GPU, 20-step Euler
ancestral, CFG 7.5 (UNet batch 8 per call), bf16 UNet, fp32-class VAE decode (pixel L-inf <= 1e-3 vs
the fp32 CPU path), synthetic name-keyed weights and synthetic conditioning (no checkpoint / CLIP
offline).  One "step" = one whole batch of images: 20 UNet calls + sampler arithmetic + VAE decode
(+ the all-gather of decoded images when N > 1).  Inputs are resident in HBM before the timed region.

    python bench.py --gpus N --steps K --warmup W
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N --steps K --warmup W

Prints ONE JSON line on rank 0.  A plain run sets up, warms up, times the K steps and prints the line (its `ms_per_step` is
one timed step); `--dump-outputs DIR` also writes what the last timed step computed, as DIR/<name>.npy.  `--full` adds what
the headline figure does not need, after the timed region: `roofline`, measured live with HIP events on the launch stream
(crg_profile_begin/end) around one extra, un-timed step; `cpu_baseline`, the CPU oracle (oracle/ref_cpu.py, "port") timed
on a bounded sample of the same workload on the host cores (rank 0, N=1); and (N=1) the SDXL 1024x1024 extra workload.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

# multi-process GPU work on this pool needs dmabuf IPC (RCCL otherwise fails with hipIpcGetMemHandle: invalid argument); the variable is
# exported by the image already - set here as well so that a bare `python -m torch.distributed.run ... bench.py` cannot miss it
os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")

import torch  # noqa: E402

REPO = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, REPO)

FLOPS_UNET_PER_SAMPLE = 803.25e9   # SD1.5 UNet call per latent sample, L=64
FLOPS_VAE_DECODE = 2514.5e9        # SD1.5 VAE decode per image, L=64
PEAK_BF16_TFLOPS = 2500.0          # dense bf16 MFMA peak, MI355X_MICROARCH.md "Chip-level parameters"
PEAK_HBM_GBS = 8000.0
DUMP_BYTES = 63 * 10**6            # --dump-outputs: bytes of array data in all (under 64 MB with the .npy headers)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--batch", type=int, default=4, help="images per GPU per step (C2: 4)")
    ap.add_argument("--sampler_steps", type=int, default=20)
    ap.add_argument("--sampler", default="euler_a")
    ap.add_argument("--workload", default="sd15", choices=["sd15", "sdxl", "img2img", "controlnet", "c5"],
                    help="sd15 = BASELINE.json configs[1] (the headline metric, default).  Extra, separately labelled measurements: "
                         "sdxl = configs[2] (SDXL 1024x1024 batch 2, 30-step Euler EDM); img2img = configs[3]'s per-GPU unit (SD1.5 "
                         "img2img 768x768, 2 images per GPU, DDIM 20 steps strength 0.75, VAE encode + decode); controlnet = "
                         "configs[1] with a ControlNet attached (SURVEY 8f row 1); c5 = configs[4]'s per-GPU unit (SDXL 1024x1024 txt2img, 1 image per GPU, then the "
                         "auto-face-fix second pass: img2img strength 0.3 on a crop brought to 1024x1024 = UNet re-entry + VAE encode + decode)")
    ap.add_argument("--no-graph", action="store_true", help="launch the UNet eagerly instead of replaying a captured hipGraph "
                                                            "(measured A/B on MI355X: replay is 0-3 %% faster and steadier)")
    ap.add_argument("--half", default="bf16", choices=["bf16", "f16"],
                    help="16-bit operand type of the UNet kernels: bf16 = the headline configuration (BASELINE.json configs[1]); f16 = the "
                         "fp16-operand build of the same kernels (libcrg_hip_f16.so, the reference's own GPU dtype) - an extra, separately labelled line")
    ap.add_argument("--unet-fp32", action="store_true",
                    help="extra line: the fp32-class UNet (fp32 activations, split-bf16 x3 MFMA) - the configuration whose 20-step trajectory "
                         "stays within 1e-3 of the fp32 CPU reference end to end (tests/test_hip_models.py::test_c1_sd15_full_20_step_trajectory)")
    ap.add_argument("--full", action="store_true",
                    help="headline workload: after the timed steps also measure the roofline / per-kernel figures, the CPU baseline and (N = 1) "
                         "the extra SDXL 1024x1024 workload; the --no-* options below drop parts of it")
    ap.add_argument("--dump-outputs", metavar="DIR", help="headline workload: write what the last timed step computed (decoded images, "
                                                          "rank 0's final latents) as DIR/<name>.npy, float32")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-extra", action="store_true", help="skip the extra SDXL 1024x1024 measurement attached to the headline line (N = 1 only)")
    ap.add_argument("--no-roofline", action="store_true")
    a = ap.parse_args()
    if a.dump_outputs and a.workload != "sd15":
        raise SystemExit("--dump-outputs covers the headline workload (--workload sd15) only")
    if a.half == "f16":
        os.environ["CRG_HALF"] = "f16"  # read by cremage_amd._lib at import: selects libcrg_hip_f16.so and torch.float16 activations

    from cremage_amd import dist as D
    from cremage_amd import ops, pipeline as P
    from cremage_amd.synth import synth_input

    if a.workload in ("sdxl", "c5"):
        return main_sdxl(a)
    if a.workload in ("img2img", "controlnet"):
        return main_extra(a)
    rank, world, local = D.init_from_env()
    if world != a.gpus:
        raise SystemExit(f"--gpus {a.gpus} but WORLD_SIZE={world}: launch with torch.distributed.run --nproc-per-node {a.gpus}")
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs a HIP device (the product path has no CPU fallback)")
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)

    # ---- model: rank 0 materialises the synthetic weights, the others receive them over RCCL ----
    t0 = time.time()
    unet_dtype = torch.float32 if a.unet_fp32 else ops.HALF
    ldm, bcast_bytes = P.build_ldm_sharded(rank, dev, unet_dtype=unet_dtype, vae_dtype=torch.float32, seed=1234)
    if not a.no_graph:
        ldm.model.enable_hip_graph(True)
    t_build = time.time() - t0

    b = a.batch
    first = rank * b  # this rank's global image indices [first, first + b)
    c = torch.stack([synth_input(f"bench.c{first + i}", (77, 768), 7) for i in range(b)]).to(dev)
    uc = synth_input("bench.uc", (1, 77, 768), 7).expand(b, -1, -1).contiguous().to(dev)
    gens = [torch.Generator(device=dev).manual_seed(D.image_seed(42, first + i)) for i in range(b)]
    last = {}

    def step(gather=True):
        # P.txt2img draws the initial latents and the ancestral noise of image i from its own generator (seed + global image index),
        # the whole trajectory's noise up front (pipeline.trajectory_noise_sampler) - the library's default path, not a bench shortcut
        images, last["latents"] = P.txt2img(ldm, c, uc, steps=a.sampler_steps, sampler=a.sampler, cfg_scale=7.5, height=512, width=512,
                                            generators=gens)
        # gather=False: the rank-0-only profiling steps behind the timed region must not enter a collective the other ranks never join
        return D.all_gather_batch(images) if gather else images

    for _ in range(a.warmup):
        step()
    D.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(a.steps):
        out = step()
    torch.cuda.synchronize()
    D.barrier()
    dt = D.max_over_ranks(time.perf_counter() - t0, dev)
    assert out.shape == (world * b, 3, 512, 512) and torch.isfinite(out).all()
    if rank == 0 and a.dump_outputs:
        dump_outputs(a.dump_outputs, {"images": out, "latents": last["latents"]})

    n_images = world * b * a.steps
    value = n_images / dt
    flops_per_image = a.sampler_steps * 2 * FLOPS_UNET_PER_SAMPLE + FLOPS_VAE_DECODE
    gm = ldm.model.graphed  # None with --no-graph
    unet_calls = a.sampler_steps * (a.warmup + a.steps)
    # `replays` counts launches of an already captured graph only: with ONE conditioning per run every UNet call but the capturing
    # one must be a replay.  A run that re-captured per step (a conditioning tensor rebuilt inside the loop) fails here.
    graph_replay = bool(gm is not None and gm.active and gm.captures == 1 and gm.replays == unet_calls - 1)
    if gm is not None and not graph_replay:  # strict capture raises; this catches a silent eager / re-capturing run all the same
        raise SystemExit(f"hipGraph replay was requested but {gm.replays} of {unet_calls} UNet calls were replays ({gm.captures} captures)")
    res = {
        "metric": "images/sec SD1.5 512x512 20-step Euler ancestral (txt2img, CFG 7.5, incl. VAE decode)",
        "value": round(value, 4), "unit": "images/s", "n_gpus": world, "steps": a.steps, "warmup": a.warmup,
        "ms_per_step": round(1e3 * dt / a.steps, 3), "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
        "dtype": "fp32-class (split-bf16 x3)" if a.unet_fp32 else ("fp16" if a.half == "f16" else "bf16"), "data": "synthetic",
        "config": {"workload": f"SD1.5 txt2img 512x512, batch 4 per GPU, 20-step Euler ancestral, {'fp32-class (fp32 activations, split-bf16 x3 MFMA)' if a.unet_fp32 else ('fp16' if a.half == 'f16' else 'bf16')} UNet (B=8 with CFG) + "
                               "fp32-class (split-bf16 x3) VAE decode, synthetic name-keyed weights, synthetic conditioning"
                               + ("" if (a.half == "bf16" and not a.unet_fp32) else "  [EXTRA line: not the headline configuration, which is the bf16 UNet]"),
                   "images_per_gpu_per_step": b, "sampler": a.sampler, "sampler_steps": a.sampler_steps, "cfg_scale": 7.5,
                   "parallelism": f"batch-sharded x{world} (weights broadcast {bcast_bytes / 1e9:.2f} GB once, images all-gathered per step)"},
        "whole_path_mfma_frac": round(value / world * flops_per_image / (PEAK_BF16_TFLOPS * 1e12), 4),
        "model_build_s": round(t_build, 1),
        # how the TIMED steps launched the UNet: true = every UNet call was one hipGraph replay (captured once per
        # conditioning; the VAE decode and the sampler arithmetic are eager launches either way)
        "graph_replay": graph_replay,
        "graph_captures": gm.captures if gm is not None else 0,
        # end-to-end error OF THE DTYPE THIS LINE TIMES against the fp32 CPU reference (reference-generated fixtures, tests/golden/):
        # the figures the GPU tests bound, measured on MI355X (tests/test_hip_models.py, CRG_TOL_REPORT=1)
        "parity": parity_of("fp32" if a.unet_fp32 else a.half),
    }

    # ---- roofline of the dominant kernel: HIP events on the launch stream, one extra un-timed step ----
    if rank == 0 and a.full and not a.no_roofline:
        ldm.model.enable_hip_graph(False)  # per-launch HIP events need eager launches (a replay is one opaque node list)
        step(gather=False)
        with ops.profile(local) as prof:
            step(gather=False)
        fam = prof.result
        res["roofline"] = roofline_of(prof.kernels)
        res["roofline"]["timed_eager"] = True  # this extra step is launched eagerly with an event pair around every kernel
        res["kernel_families_ms_per_step"] = {k: round(v["ms"], 3) for k, v in fam.items() if v["launches"]}
        res["kernel_families_tflops_or_gbs"] = {
            k: (round(v["flops"] / (v["ms"] * 1e-3) / 1e12, 1) if k in ("gemm", "conv", "attention") else round(v["bytes"] / (v["ms"] * 1e-3) / 1e9, 1))
            for k, v in fam.items() if v["launches"] and v["ms"] > 0}

    # ---- CPU baseline: the oracle ("port") on a bounded sample of the same workload ----
    if rank == 0 and world == 1 and a.full and not a.no_cpu_baseline:
        from oracle import ref_cpu as R
        usd = {k: v.detach().float().cpu() for k, v in ldm.model.diffusion_model.state_dict().items()}
        vsd = {k: v.detach().float().cpu() for k, v in ldm.first_stage_model.state_dict().items()}
        x = synth_input("bench.cpu.x", (2, 4, 64, 64), 1)
        ctx = torch.cat([uc[:1].float().cpu(), c[:1].float().cpu()])
        tt = torch.tensor([500.25, 500.25])
        with torch.no_grad():
            t0 = time.perf_counter()
            R.unet_forward(usd, P.SD15_UNET, x, tt, ctx)
            t_unet = time.perf_counter() - t0
            t0 = time.perf_counter()
            R.decode_first_stage(vsd, P.SD15_VAE_DD, x[:1])
            t_dec = time.perf_counter() - t0
        res["cpu_baseline"] = {"value": round(1.0 / (a.sampler_steps * t_unet + t_dec), 6), "unit": "images/s",
                               "cores": torch.get_num_threads(), "kind": "port",
                               "sample": f"1 UNet call (B=2 = one image x CFG, 64x64 latent, fp32) = {t_unet:.2f} s and 1 VAE decode = "
                                         f"{t_dec:.2f} s on the host; images/s = 1 / (20 * t_unet + t_dec)"}
    # ---- the 1024x1024 workload (BASELINE.json configs[2], north_star "512x512 and 1024x1024") in the same record ----
    if rank == 0 and world == 1 and a.full and not a.no_extra and a.half == "bf16" and not a.unet_fp32:
        t_extra = time.time()
        try:
            import gc
            ldm.model.enable_hip_graph(False)  # drop the captured graphs and their pools; the SD1.5 weights (4 GB of 288) may stay
            gc.collect()
            ops.clear_weight_cache()
            torch.cuda.empty_cache()
            res["extra_workloads"] = {"sdxl_1024": run_sdxl(a, rank, world, local, warmup=1, steps_timed=2, c5=False, budget_s=240.0)}
        except BaseException as e:  # never let the extra line touch the headline
            res["extra_workloads"] = {"sdxl_1024": {"error": f"{type(e).__name__}: {e}"[:300]}}
        res["extra_workloads"]["seconds"] = round(time.time() - t_extra, 1)
    if rank == 0:
        print(json.dumps(res))
    if world > 1:
        torch.distributed.destroy_process_group()


def dump_outputs(path, arrays):
    """Write each tensor of `arrays` as <path>/<name>.npy in float32.  Above DUMP_BYTES in all, every array keeps the same share of
    its flattened elements, drawn with a fixed seed: the same elements on every run with the same arguments."""
    os.makedirs(path, exist_ok=True)
    arrs = {k: v.detach().float().cpu().numpy() for k, v in arrays.items()}
    total = sum(x.nbytes for x in arrs.values())
    for k, x in arrs.items():
        if total > DUMP_BYTES:
            keep = x.size * DUMP_BYTES // total
            x = x.reshape(-1)[np.sort(np.random.RandomState(0).choice(x.size, keep, replace=False))]
        np.save(os.path.join(path, k + ".npy"), x)


# End-to-end error of each UNet operand type against the fp32 CPU reference: full-size C1 (SD1.5 512x512, 20-step Euler, CFG 7.5, one
# image; reference-run fixture traj_c1_sd15_full.npz), measured on MI355X and bounded at 1.5x by tests/test_hip_models.py
# (test_c1_sd15_full_20_step_trajectory, test_fp16_operand_build, test_vae_sd15_full_decode_pixels).  Pixels in [-1, 1].
PARITY = {  # as measured with this round's kernels (gpurun_out/r4_tol.log, CRG_TOL_REPORT=1)
    "bf16": {"c1_latent_rel_l2": 6.4e-2, "c1_pixel_linf": 0.132, "c1_pixel_mean_abs": 1.5e-2},
    "f16": {"c1_latent_rel_l2": 8.3e-3, "c1_pixel_linf": 1.6e-2, "c1_pixel_mean_abs": 2.0e-3},
    "fp32": {"c1_latent_rel_l2": 9.3e-5, "c1_pixel_linf": 3.0e-4, "c1_pixel_mean_abs": 3.9e-5},
}


def parity_of(kind):
    d = dict(PARITY[kind])
    d.update({"dtype": {"bf16": "bf16", "f16": "fp16", "fp32": "fp32-class (split-bf16 x3)"}[kind] + " UNet + fp32-class VAE",
              "vae_pixel_linf": 2.0e-5, "unet_call_rel_l2": {"bf16": 1.5e-2, "f16": 2.0e-3, "fp32": 2.0e-5}[kind],
              "reference": "modules/ldm CPU fp32 (fixtures generated by oracle/gen_golden.py from the reference's own modules)",
              "bounded_by": "tests/test_hip_models.py::test_c1_sd15_full_20_step_trajectory, ::test_fp16_operand_build, ::test_vae_sd15_full_decode_pixels, ::test_unet_sd15_full",
              "note": "north_star's 1e-3 pixel bound is stated for the VAE decode (met: 2.0e-5); over the whole 20-step trajectory only the fp32-class UNet stays inside 1e-3"})
    return d


def committed_traffic(slot):
    """HBM bytes per launch of a kernel slot from the newest committed PMC summary (profiles/*_by_slot.json, written by
    tools/summarize_profile.py from separate `rocprofv3 --pmc FETCH_SIZE` / `--pmc WRITE_SIZE` passes of this same
    command).  Counters cannot be collected from inside this process, so this is the per-launch figure of that run."""
    import glob
    for path in sorted(glob.glob(os.path.join(os.path.dirname(os.path.abspath(__file__)), "profiles", "*_by_slot.json")), reverse=True):
        try:
            e = json.load(open(path)).get(slot)
        except Exception:
            continue
        if e and e.get("hbm_bytes_per_launch"):
            return float(e["hbm_bytes_per_launch"]), os.path.basename(path)
    return None, None


def roofline_of(kernels):
    """`roofline` object for the dominant kernel (largest summed device time) of one profiled step."""
    dom = max(kernels, key=lambda k: kernels[k]["ms"])
    k = kernels[dom]
    mfma = k["family"] in ("gemm", "conv", "attention")
    n = max(1, k["launches"])
    if mfma:
        ach, peak, unit = k["flops"] / (k["ms"] * 1e-3) / 1e12, PEAK_BF16_TFLOPS, "TFLOP/s"
    else:
        ach, peak, unit = k["bytes"] / (k["ms"] * 1e-3) / 1e9, 8000.0, "GB/s"
    traffic, src = committed_traffic(dom)
    return {"kernel": k["symbol"], "slot": dom, "bound": "mfma" if mfma else "hbm", "achieved": round(ach, 2), "peak": peak, "unit": unit,
            "frac": round(ach / peak, 4), "traffic": traffic, "traffic_source": src, "launches": k["launches"],
            "avg_launch_us": round(1e3 * k["ms"] / n, 2), "algorithmic_gflop_per_launch": round(k["flops"] / n / 1e9, 3),
            "algorithmic_mbytes_per_launch": round(k["bytes"] / n / 1e6, 3),
            "kernels_ms_per_step": {name: round(v["ms"], 3) for name, v in kernels.items() if v["launches"]},
            # per slot: launches and ALGORITHMIC work per launch (FLOPs = 2 MAC of the op; bytes = operands + result once)
            "kernels_per_launch": {name: {"launches": v["launches"], "us": round(1e3 * v["ms"] / v["launches"], 2),
                                          "gflop": round(v["flops"] / v["launches"] / 1e9, 3),
                                          "mbytes": round(v["bytes"] / v["launches"] / 1e6, 3)}
                                   for name, v in kernels.items() if v["launches"]}}


def main_extra(a):
    """Extra SD1.5 workloads on the same path (same sharding and timing protocol as the headline run)."""
    from cremage_amd import dist as D
    from cremage_amd import ops, pipeline as P
    from cremage_amd.synth import synth_input
    rank, world, local = D.init_from_env()
    if world != a.gpus:
        raise SystemExit(f"--gpus {a.gpus} but WORLD_SIZE={world}: launch with torch.distributed.run --nproc-per-node {a.gpus}")
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    t0 = time.time()
    if a.workload == "controlnet":
        ldm = P.build_synthetic_control_ldm(device=dev)
        b, hw = a.batch, 512
    else:
        ldm = P.build_synthetic_ldm(device=dev)
        b, hw = (2 if a.batch == 4 else a.batch), 768
    D.broadcast_module_(ldm, src=0)  # every rank filled the same name-keyed weights; the broadcast makes rank 0 authoritative
    t_build = time.time() - t0
    L = hw // 8
    first = rank * b
    c = torch.stack([synth_input(f"bench.c{first + i}", (77, 768), 7) for i in range(b)]).to(dev)
    uc = synth_input("bench.uc", (1, 77, 768), 7).expand(b, -1, -1).contiguous().to(dev)
    gens = [torch.Generator(device=dev).manual_seed(D.image_seed(42, first + i)) for i in range(b)]
    rnd = lambda shape: torch.stack([torch.randn(shape, generator=g, device=dev) for g in gens])
    if a.workload == "controlnet":
        hint = torch.stack([synth_input(f"bench.hint{first + i}", (3, hw, hw), 44, 0.5) for i in range(b)]).clamp(-1, 1).mul(0.5).add(0.5).to(dev)

        def step(gather=True):
            images, _ = P.txt2img(ldm, c, uc, steps=a.sampler_steps, sampler=a.sampler, cfg_scale=7.5, height=hw, width=hw,
                                  x0=rnd((4, L, L)), noise_sampler=lambda s, sn: rnd((4, L, L)), hint=hint)
            return D.all_gather_batch(images) if gather else images
        # ControlNet = encoder half + middle of the UNet + hint encoder: FLOPs counted by the profiler below, not assumed
        metric = "images/sec SD1.5 512x512 20-step Euler ancestral + ControlNet (txt2img, CFG 7.5, incl. VAE decode)"
        workload = ("SD1.5 txt2img 512x512 with a ControlNet (cldm_v15.yaml), batch 4 per GPU, 20-step Euler ancestral, bf16 UNet + "
                    "ControlNet (B=8 with CFG), fp32-class VAE decode, synthetic weights / conditioning / hint")
        flops_per_image = None
    else:
        img = torch.stack([synth_input(f"bench.img{first + i}", (3, hw, hw), 44, 0.5) for i in range(b)]).clamp(-1, 1).to(dev)

        def step(gather=True):
            images, _ = P.img2img(ldm, img, c, uc, steps=a.sampler_steps, strength=0.75, cfg_scale=7.5, enc_noise=rnd((4, L, L)),
                                  fwd_noise=rnd((4, L, L)))
            return D.all_gather_batch(images) if gather else images
        metric = "images/sec SD1.5 img2img 768x768 20-step DDIM strength 0.75 (VAE encode + 15 UNet steps x CFG + VAE decode)"
        workload = ("SD1.5 img2img 768x768 (BASELINE.json configs[3] per-GPU unit), 2 images per GPU, DDIM 20 steps, strength 0.75 -> "
                    "t_enc 15, bf16 UNet (B=4 with CFG, L=96), fp32-class VAE encode + decode, synthetic weights / inputs")
        flops_per_image = 2609.1e9 + 30 * 2148.1e9 + 5754.3e9  # enc 768^2 + 15 x 2 x UNet(L=96) + dec(L=96)
    for _ in range(a.warmup):
        step()
    D.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(a.steps):
        out = step()
    torch.cuda.synchronize()
    D.barrier()
    dt = D.max_over_ranks(time.perf_counter() - t0, dev)
    assert out.shape == (world * b, 3, hw, hw) and torch.isfinite(out).all()
    value = world * b * a.steps / dt
    res = {"metric": metric, "value": round(value, 4), "unit": "images/s", "n_gpus": world, "steps": a.steps, "warmup": a.warmup,
           "ms_per_step": round(1e3 * dt / a.steps, 3), "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "bf16",
           "data": "synthetic", "config": {"workload": workload, "images_per_gpu_per_step": b, "sampler_steps": a.sampler_steps},
           "model_build_s": round(t_build, 1)}
    if rank == 0 and not a.no_roofline:
        with ops.profile(local) as prof:
            step(gather=False)  # rank 0 only: no collective in here
        fam = prof.result
        res["roofline"] = roofline_of(prof.kernels)
        res["roofline"]["traffic"] = res["roofline"]["traffic_source"] = None  # the committed PMC passes are of the headline workload
        res["kernel_families_ms_per_step"] = {k: round(v["ms"], 3) for k, v in fam.items() if v["launches"]}
        total_flops = sum(v["flops"] for k, v in fam.items() if k in ("gemm", "conv", "attention", "conv_small"))
        res["algorithmic_gflop_per_image"] = round((flops_per_image if flops_per_image else total_flops / b) / 1e9, 1)
        res["whole_path_mfma_frac"] = round(value / world * res["algorithmic_gflop_per_image"] * 1e9 / (PEAK_BF16_TFLOPS * 1e12), 4)
    if rank == 0:
        print(json.dumps(res))
    if world > 1:
        torch.distributed.destroy_process_group()


def main_sdxl(a):
    """BASELINE.json configs[2]: SDXL txt2img 1024x1024 base-only, batch 2 per GPU, 30-step Euler (EDM), bf16 UNet + fp32-class VAE."""
    from cremage_amd import dist as D
    rank, world, local = D.init_from_env()
    res = run_sdxl(a, rank, world, local, warmup=a.warmup, steps_timed=a.steps, c5=a.workload == "c5", roofline=not a.no_roofline)
    if rank == 0:
        print(json.dumps(res))
    if world > 1:
        torch.distributed.destroy_process_group()


def run_sdxl(a, rank, world, local, warmup, steps_timed, c5, roofline=True, budget_s=None):
    """One measurement of the SDXL path (same sharding and timing protocol as the headline run); returns the record.  `budget_s`: give up
    (RuntimeError) before the timed region when building + warming up already used that much wall time."""
    from cremage_amd import dist as D
    from cremage_amd import ops, pipeline as P
    from cremage_amd.synth import synth_input
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    b = (1 if c5 else 2) if a.batch == 4 else a.batch
    steps = 30 if a.sampler_steps == 20 else a.sampler_steps
    t_start = t0 = time.time()
    eng = P.build_synthetic_sdxl(device=dev, fill=(rank == 0))
    D.broadcast_module_(eng, src=0)
    t_build = time.time() - t0
    first = rank * b
    c = {"crossattn": torch.stack([synth_input(f"bench.xl.c{first + i}", (77, 2048), 7) for i in range(b)]).to(dev),
         "vector": torch.stack([synth_input(f"bench.xl.v{first + i}", (2816,), 7) for i in range(b)]).to(dev)}
    uc = {"crossattn": synth_input("bench.xl.uc", (1, 77, 2048), 7).expand(b, -1, -1).contiguous().to(dev),
          "vector": synth_input("bench.xl.ucv", (1, 2816), 7).expand(b, -1).contiguous().to(dev)}
    gens = [torch.Generator(device=dev).manual_seed(D.image_seed(42, first + i)) for i in range(b)]

    def step(gather=True):
        x0 = torch.stack([torch.randn((4, 128, 128), generator=g, device=dev) for g in gens])
        if c5:  # first pass, then the face-fix re-entry on a fixed 512x512 box brought to 1024x1024 (one "face" per image)
            rn = lambda: torch.stack([torch.randn((4, 128, 128), generator=g, device=dev) for g in gens])
            images, _, _ = P.txt2img_sdxl_facefix(eng, c, uc, [(256, 256, 512)] * b, steps=steps, cfg_scale=5.0, x0=x0, strength=0.3,
                                                  enc_noise=rn(), fwd_noise=rn())
        else:
            images, _ = P.txt2img_sdxl(eng, c, uc, steps=steps, cfg_scale=5.0, x0=x0)
        return D.all_gather_batch(images) if gather else images

    for _ in range(warmup):
        step()
    D.barrier()
    torch.cuda.synchronize()
    if budget_s is not None and time.time() - t_start > budget_s:
        raise RuntimeError(f"build + warm-up took {time.time() - t_start:.0f} s of a {budget_s:.0f} s budget: not timed")
    t0 = time.perf_counter()
    for _ in range(steps_timed):
        out = step()
    torch.cuda.synchronize()
    D.barrier()
    dt = D.max_over_ranks(time.perf_counter() - t0, dev)
    assert out.shape == (world * b, 3, 1024, 1024) and torch.isfinite(out).all()
    value = world * b * steps_timed / dt
    flops_per_image = steps * 2 * 6760e9 + 10470.4e9
    metric = "images/sec SDXL 1024x1024 base-only 30-step Euler EDM (txt2img, CFG 5, incl. VAE decode)"
    workload = ("SDXL txt2img 1024x1024 base-only, batch 2 per GPU, 30-step Euler EDM, bf16 UNet (B=4 with CFG) + "
                "fp32-class VAE decode, synthetic weights/conditioning (BASELINE.json configs[2])")
    if c5:
        n2 = max(int(0.3 * (steps + 1)), 1) - 1  # UNet steps of the second pass: the pruned schedule keeps int(0.3 * (steps + 1)) sigmas
        # + VAE encode at 1024^2 (4 x the 512^2 figure of SURVEY 8d: conv-only encoder) + n2 x 2 UNet calls + a second decode
        flops_per_image += 4 * 1116.7e9 + n2 * 2 * 6760e9 + 10470.4e9
        metric = "images/sec SDXL 1024x1024 30-step Euler EDM + auto-face-fix second pass (img2img strength 0.3 on a crop, UNet re-entry)"
        workload = (f"SDXL txt2img 1024x1024 + face-fix re-entry (BASELINE.json configs[4] per-GPU unit): {b} image per GPU, 30-step Euler EDM, "
                    f"then a fixed 512x512 box resized to 1024x1024 -> VAE encode -> {n2} Euler-EDM steps (strength 0.3) x CFG -> VAE decode "
                    "-> paste; bf16 UNet, fp32-class VAE; box instead of the face detector, bilinear instead of cv2 Lanczos (out of scope)")
    res = {"metric": metric, "value": round(value, 4),
           "unit": "images/s", "n_gpus": world, "steps": steps_timed, "warmup": warmup, "ms_per_step": round(1e3 * dt / steps_timed, 3),
           "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "bf16", "data": "synthetic",
           "config": {"workload": workload, "images_per_gpu_per_step": b, "sampler_steps": steps},
           "whole_path_mfma_frac": round(value / world * flops_per_image / (PEAK_BF16_TFLOPS * 1e12), 4), "model_build_s": round(t_build, 1),
           "parity_ref": "tests/test_hip_models.py::test_sgm_unet_sdxl_full (2.57 B parameters, bf16 rel-L2 1.7e-2 vs the reference's own sgm UNetModel on the "
                         "CPU, bound 3.3e-2), ::test_sgm_vae_full_decode_1024 (pixel L-inf 1.5e-5), ::test_sdxl_trajectory_euler_edm"}
    if rank == 0 and roofline:
        with ops.profile(local) as prof:
            step(gather=False)  # rank 0 only: no collective in here
        fam = prof.result
        res["roofline"] = roofline_of(prof.kernels)
        res["roofline"]["traffic"] = res["roofline"]["traffic_source"] = None  # the committed PMC passes are of the SD1.5 workload
        res["kernel_families_ms_per_step"] = {k: round(v["ms"], 3) for k, v in fam.items() if v["launches"]}
        res["kernel_families_tflops_or_gbs"] = {
            k: (round(v["flops"] / (v["ms"] * 1e-3) / 1e12, 1) if k in ("gemm", "conv", "attention") else round(v["bytes"] / (v["ms"] * 1e-3) / 1e9, 1))
            for k, v in fam.items() if v["launches"] and v["ms"] > 0}
    return res


if __name__ == "__main__":
    main()
