#!/usr/bin/env python
"""Cost of the spot-inpainting glue for a 1024 x 1024 and a 512 x 512 image, one GPU process, device events around the glue, medians
over `--reps` (default 20) repetitions after a warm-up.

Prints one JSON line; per image size `hw`:
  blend_ms_full / blend_ms_window      crg_blur_blend_u8 alone, in place: the whole image, and with window = the mask's dilated box
  composite_ms_host                    the host composite of an image that lives on the device: device -> host copy of the two
                                       images, postprocess.blend_blurred_mask in numpy, host -> device copy of the result
  composite_ms_device                  postprocess.blend_blurred_mask_device with the window (mask already on the device)
  spot_box_ms_host / _device           one spot-fix box end to end (SD1.5 at 512 x 512, bf16 UNet, 20 DDIM steps at strength 0.5) with
                                       resample="host" / "device"
  img2img_ms_host / _device            the img2img call inside those runs
  glue_ms_host / _device               the difference of the two medians
`--no-model` skips the spot-fix rows (no UNet is built)."""
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cremage_amd import ops  # noqa: E402
from cremage_amd import pipeline as P  # noqa: E402
from cremage_amd import postprocess as PP  # noqa: E402
from cremage_amd.synth import synth_input  # noqa: E402


def timed(fn, reps, warmup=3):
    """median ms of fn() between two events; the host waits for the second one, so host-side work in fn counts"""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return statistics.median(ms)


def spot_mask(hw):
    """one blob of hw/8 x hw/6 pixels right of the centre"""
    m = np.zeros((hw, hw), np.uint8)
    m[hw // 2:hw // 2 + hw // 8, hw // 2:hw // 2 + hw // 6] = 255
    return m


def glue_rows(hw, reps, dev):
    rng = np.random.RandomState(hw)
    orig = torch.from_numpy(rng.randint(0, 256, (hw, hw, 3)).astype(np.uint8)).to(dev)
    upd = torch.from_numpy(rng.randint(0, 256, (hw, hw, 3)).astype(np.uint8)).to(dev)
    mask = spot_mask(hw)
    mask_dev = torch.from_numpy(mask).to(dev)
    window = PP.mask_window(mask)
    work = orig.clone()
    out = dict(hw=hw, window=list(window))
    out["blend_ms_full"] = round(timed(lambda: ops.blur_blend_u8(work, upd, mask_dev, out=work), reps), 4)
    out["blend_ms_window"] = round(timed(lambda: ops.blur_blend_u8(work, upd, mask_dev, out=work, window=window), reps), 4)

    def host():
        res = PP.blend_blurred_mask(orig.cpu().numpy(), upd.cpu().numpy(), mask)
        return torch.from_numpy(res).to(dev)
    out["composite_ms_host"] = round(timed(host, reps), 3)
    out["composite_ms_device"] = round(timed(lambda: PP.blend_blurred_mask_device(orig, upd, mask_dev, window=window), reps), 4)
    assert torch.equal(host(), PP.blend_blurred_mask_device(orig, upd, mask_dev, window=window))
    return out


def spot_rows(ldm, hw, reps, dev):
    image = torch.from_numpy(np.random.RandomState(hw + 1).rand(3, hw, hw).astype(np.float32)).to(dev)
    mask = spot_mask(hw)
    c, uc = synth_input("st.c", (1, 77, 768), 1).to(dev), synth_input("st.uc", (1, 77, 768), 1).to(dev)
    en, fn = synth_input("st.en", (1, 4, 64, 64), 1).to(dev), synth_input("st.fn", (1, 4, 64, 64), 1).to(dev)
    inner = []
    real = P.img2img

    def probe(*a, **kw):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        r = real(*a, **kw)
        e1.record()
        inner.append((e0, e1))
        return r
    out, res = {}, {}
    P.img2img = probe
    try:
        for arm in P.RESAMPLERS:
            def run(arm=arm):
                res[arm] = P.spot_fix_sd15(ldm, image, mask, c, uc, steps=20, strength=0.5, resample=arm, enc_noise=en, fwd_noise=fn)
            run()
            inner.clear()
            total = timed(run, reps, warmup=1)
            torch.cuda.synchronize()
            i2i = statistics.median([a.elapsed_time(b) for a, b in inner[-reps:]])
            out[f"spot_box_ms_{arm}"], out[f"img2img_ms_{arm}"], out[f"glue_ms_{arm}"] = round(total, 2), round(i2i, 2), round(total - i2i, 2)
    finally:
        P.img2img = real
    out["arms_equal"] = bool(torch.equal(res["host"], res["device"]))
    return out


def main():
    reps = int(sys.argv[sys.argv.index("--reps") + 1]) if "--reps" in sys.argv else 20
    if reps < 20:
        raise SystemExit("--reps must be at least 20")
    dev = torch.device("cuda:0")
    rows = [glue_rows(hw, reps, dev) for hw in (1024, 512)]
    if "--no-model" not in sys.argv:
        ldm = P.build_synthetic_ldm(device=dev, seed=1)
        with torch.no_grad():
            for row in rows:
                row.update(spot_rows(ldm, row["hw"], reps, dev))
    print(json.dumps(dict(reps=reps, device=torch.cuda.get_device_name(0), rows=rows)), flush=True)


if __name__ == "__main__":
    main()
