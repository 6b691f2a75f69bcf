"""Times the gradient-domain ("poisson") face paste on the host (postprocess.poisson_clone_host, float64 numpy) against the device
(ops.poisson_clone), one JSON line per item.

  python tools/poisson_time.py glue      one face-fix glue round (crop -> resize -> pad, un-pad -> resize -> poisson paste) at 1024^2 with a
                                         300 x 340 face (a 380 x 340 patch), paste_mode="poisson" on the host against the device
  python tools/poisson_time.py solve     ops.poisson_clone alone (the right-hand-side kernel and the four fp32 MFMA products) at the
                                         380 x 340 patch and at the largest patch a 1024^2 image allows (1024 x 1024), device events
                                         around each call; the FLOP count is the four products', 2 * 3 * n * m * (2 n + 2 m)
  python tools/poisson_time.py kernel    the calls of `solve` only, a few times each: run it under
                                         `rocprofv3 --kernel-trace --stats -- python tools/poisson_time.py kernel` for each kernel's own time

`glue`: every figure is ONE call; the arms alternate in three pairs (host, device, host, device, ...) after one untimed call of each,
and every timed window ends with a device synchronise inside it.  The two arms do not return the same bytes (the device solves in
fp32): the line reports how many bytes differ and the largest difference instead of bit equality.  These are records for DESIGN f11,
not pass or fail figures."""
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from cremage_amd import ops  # noqa: E402
from cremage_amd import pipeline as P  # noqa: E402
from cremage_amd import postprocess as PP  # noqa: E402

DEV = "cuda:0"
PAIRS = 3
PATCHES = ((380, 340), (1024, 1024))  # (h, w)


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def stand_in(x):
    return (x.to(DEV) + 1.0) * 0.5  # [-1, 1] -> [0, 1]: the glue round without the UNet pass


def glue():
    g = torch.Generator().manual_seed(0)
    big, faces = torch.rand((3, 1024, 1024), generator=g).to(DEV), [(400, 300, 300, 340)]
    arms = {"host": lambda: P._face_fix_one(PP, big, faces, stand_in, 1024, "host", "poisson").to(DEV),
            "device": lambda: P._face_fix_one(PP, big, faces, stand_in, 1024, "device", "poisson")}
    for fn in arms.values():  # untimed: tables, allocator, PIL import
        fn()
    ms, outs = {"host": [], "device": []}, {}
    for _ in range(PAIRS):
        for arm, fn in arms.items():
            t, outs[arm] = timed(fn)
            ms[arm].append(round(t, 3))
    diff = ((outs["host"] - outs["device"]).abs() * 255.0).round()
    print(json.dumps({"item": "face-fix glue round 1024^2, face 300x340, paste_mode poisson", "host_ms": ms["host"], "device_ms": ms["device"],
                      "bytes_differing": int((diff != 0).sum()), "max_byte_difference": int(diff.max())}), flush=True)


def _solve_inputs(h, w):
    g = torch.Generator().manual_seed(h + w)
    image = (torch.rand((1, 3, 1024, 1024), generator=g) * 255.0).to(torch.uint8).to(DEV)
    patch = (torch.rand((1, 3, h, w), generator=g) * 255.0).to(torch.uint8).to(DEV)
    return image, patch, ((1024 - w) // 2, (1024 - h) // 2)


def solve():
    for h, w in PATCHES:
        image, patch, off = _solve_inputs(h, w)
        ops.poisson_clone(image.clone(), patch, off)  # untimed: tables
        ms = []
        for _ in range(5):
            work = image.clone()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            ops.poisson_clone(work, patch, off)
            e1.record()
            torch.cuda.synchronize()
            ms.append(round(e0.elapsed_time(e1), 4))
        n, m = h - 4, w - 4
        gflop = 2.0 * 3 * n * m * (2 * n + 2 * m) / 1e9
        print(json.dumps({"item": f"ops.poisson_clone, patch {h}x{w} in 1024^2 (5 launches per call)", "ms": ms, "gflop": round(gflop, 3),
                          "tflops_at_min": round(gflop / min(ms), 2)}), flush=True)


def kernel():
    for h, w in PATCHES:
        image, patch, off = _solve_inputs(h, w)
        for _ in range(5):
            ops.poisson_clone(image.clone(), patch, off)
    torch.cuda.synchronize()


if __name__ == "__main__":
    what = sys.argv[1] if len(sys.argv) > 1 else "glue"
    {"glue": glue, "solve": solve, "kernel": kernel}[what]()
