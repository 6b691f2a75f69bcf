"""Times the pixel-space Lanczos glue on the host (PIL, the default) against the device (ops.resample_u8), one JSON line per item.

  python tools/resample_time.py glue      upscale_uint8 vs upscale_uint8_device at 4 x 3 x 512^2 -> 1024^2, and one face-fix glue round
                                          (crop -> resize -> pad, un-pad -> resize -> paste) at 1024^2 with a 300 x 340 face
  python tools/resample_time.py e2e       SD1.5 txt2img_hires(upscaler="lanczos"), 4 x 512^2 -> 1024^2, 20 steps, resample= host vs device
  python tools/resample_time.py kernel    the device calls of `glue` only, a few times each: run it under
                                          `rocprofv3 --kernel-trace --stats -- python tools/resample_time.py kernel` for the kernel's own time

Every figure is ONE call; the arms alternate in three pairs (host, device, host, device, ...) after one untimed call of each, and every
timed window ends with a device synchronise inside it.  "host" is the code path of the package without this keyword: the baseline."""
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from cremage_amd import pipeline as P  # noqa: E402
from cremage_amd import postprocess as PP  # noqa: E402

DEV = "cuda:0"
PAIRS = 3


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def pairs(name, host, device, same=None):
    host(), device()  # untimed: tables, allocator, PIL import
    ms = {"host": [], "device": []}
    for _ in range(PAIRS):
        for arm, fn in (("host", host), ("device", device)):
            t, out = timed(fn)
            ms[arm].append(round(t, 3))
            ms.setdefault("_out", {})[arm] = out
    outs = ms.pop("_out")
    equal = bool(same(outs["host"], outs["device"])) if same else None
    print(json.dumps({"item": name, "host_ms": ms["host"], "device_ms": ms["device"], "bit_equal": equal}), flush=True)


def stand_in(x):
    return (x.to(DEV) + 1.0) * 0.5  # [-1, 1] -> [0, 1]: the glue round without the UNet pass


def glue_inputs():
    g = torch.Generator().manual_seed(0)
    return torch.rand((4, 3, 512, 512), generator=g).to(DEV), torch.rand((3, 1024, 1024), generator=g).to(DEV), [(400, 300, 300, 340)]


def glue():
    imgs, big, faces = glue_inputs()
    pairs("upscale_uint8 4x3x512^2 -> 1024^2", lambda: PP.upscale_uint8(imgs, 1024, 1024), lambda: PP.upscale_uint8_device(imgs, 1024, 1024),
          torch.equal)
    pairs("face-fix glue round 1024^2, face 300x340", lambda: P._face_fix_one(PP, big, faces, stand_in, 1024, "host").to(DEV),
          lambda: P._face_fix_one(PP, big, faces, stand_in, 1024, "device"), torch.equal)


def kernel():
    imgs, big, faces = glue_inputs()
    for _ in range(5):
        PP.upscale_uint8_device(imgs, 1024, 1024)
        P._face_fix_one(PP, big, faces, stand_in, 1024, "device")
    torch.cuda.synchronize()


def e2e():
    ldm = P.build_synthetic_ldm(device=DEV)
    g = torch.Generator().manual_seed(0)
    c, uc = torch.randn((4, 77, 768), generator=g).to(DEV), torch.randn((4, 77, 768), generator=g).to(DEV)
    x0 = torch.randn((4, 4, 64, 64), generator=g).to(DEV)
    en, fn = torch.randn((4, 4, 128, 128), generator=g).to(DEV), torch.randn((4, 4, 128, 128), generator=g).to(DEV)

    def run(resample):
        return P.txt2img_hires(ldm, c, uc, steps=20, sampler="euler", height=512, width=512, factor=2.0, strength=0.5, x0=x0, fwd_noise=fn,
                               enc_noise=en, upscaler="lanczos", resample=resample)[0]
    pairs("SD1.5 txt2img_hires lanczos 4 x 512^2 -> 1024^2, 20 steps", lambda: run("host"), lambda: run("device"), torch.equal)


if __name__ == "__main__":
    what = sys.argv[1] if len(sys.argv) > 1 else "glue"
    {"glue": glue, "e2e": e2e, "kernel": kernel}[what]()
