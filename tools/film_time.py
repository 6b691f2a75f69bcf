"""Device time of the FILM interpolator at the Video Generator's size (1024 x 576, batch 1, the film_net configuration, fp32 class):

  * every kernel of film.hip at the shapes of the finest pyramid level, replayed from a captured hipGraph (median of the replays, random
    data), with the bytes the operation has to move - one read of what it reads, one write of what it writes - over that time, next to the
    same operation composed from PyTorch-ROCm fp32 ops (tests/_film_cases.py);
  * one Interpolator call against the same restatement of the whole network on PyTorch-ROCm fp32, in alternating pairs inside one
    process (device events around each call, both warmed up), plus the HIP call's device time per kernel family.

    python tools/film_time.py [--reps 20] [--pairs 5] [--hw 576 1024] [--skip-model]
Prints one JSON line per measurement.  Nothing is asserted."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from cremage_amd import ops  # noqa: E402
from tests import _film_cases as FC  # noqa: E402
from tools.svd_time import graph_ms  # noqa: E402

DEV = "cuda:0"


def out(**kw):
    print(json.dumps(kw), flush=True)


def cl(*shape):
    n, c, h, w = shape
    return torch.randn(n, h, w, c, device=DEV).permute(0, 3, 1, 2)


def row(what, reps, fn, base, gbytes, **kw):
    a, b = graph_ms(fn, reps), graph_ms(base, reps)
    out(what=what, ms=a[0], ms_min=a[1], gb=gbytes, gb_per_s=gbytes / a[0] * 1e3, torch_ms=b[0], torch_ms_min=b[1], **kw)


def kernel_rows(reps, H, W):
    C = 64  # feature channels of the finest level; its fusion input is 2 (3 + 64) + 4 = 138 columns, rounded up to 144 with the 64 of the coarser level
    px = H * W
    feat, img = cl(1, C, H, W), cl(1, 3, H, W)
    flow = cl(1, 2, H, W) * 4.0
    s = torch.full((1,), 0.5, device=DEV)
    buf = ops.empty_image(1, 208, H, W, torch.float32, DEV)
    both = torch.cat([img, feat], 1).contiguous(memory_format=torch.channels_last)
    row("warp_flow C=64 into a slice at column 3", reps, lambda: ops.warp_flow(feat, flow, s, out=buf[:, 3:3 + C]), lambda: FC.warp(feat, flow, s),
        px * (2 * C + 2) * 4e-9, C=C, hw=[H, W])
    row("warp_flow C=3 into a slice at column 0", reps, lambda: ops.warp_flow(img, flow, s, out=buf[:, 0:3]), lambda: FC.warp(img, flow, s),
        px * (2 * 3 + 2) * 4e-9, C=3, hw=[H, W])
    out(what="torch: warp of cat([image, features]) C=67 (what the reference launches)", torch_ms=graph_ms(lambda: FC.warp(both, flow, s), reps)[0])
    dense = ops.empty_image(1, C, H, W, torch.float32, DEV)
    row("warp_flow C=64 dense", reps, lambda: ops.warp_flow(feat, flow, s, out=dense), lambda: FC.warp(feat, flow, s), px * (2 * C + 2) * 4e-9, C=C, hw=[H, W])
    row("avg_pool2 C=64", reps, lambda: ops.avg_pool2(feat), lambda: FC.avg_pool2(feat), px * C * 1.25 * 4e-9, C=C, hw=[H, W])
    row("avg_pool2 C=3", reps, lambda: ops.avg_pool2(img), lambda: FC.avg_pool2(img), px * 3 * 1.25 * 4e-9, C=3, hw=[H, W])
    v, res = cl(1, 2, H // 2, W // 2), cl(1, 2, H, W)
    row("flow_up2_add with residual", reps, lambda: ops.flow_up2_add(v, res), lambda: FC.flow_up2_add(v, res), px * 2 * 2.25 * 4e-9, hw=[H, W])
    row("flow_up2_add", reps, lambda: ops.flow_up2_add(v), lambda: FC.flow_up2_add(v), px * 2 * 1.25 * 4e-9, hw=[H, W])
    y = cl(1, C, H, W)
    big = ops.empty_image(1, 2 * C, H, W, torch.float32, DEV)
    row("leaky_split fp32 into a slice", reps, lambda: ops.leaky_split(y, 0.2, out=big[:, :C]), lambda: FC.leaky(y), px * C * 2 * 4e-9, C=C, hw=[H, W])
    row("leaky_split fp32 into a slice + 2x2 mean", reps, lambda: ops.leaky_split(y, 0.2, out=big[:, :C], pool=True), lambda: FC.avg_pool2(FC.leaky(y)),
        px * C * 2.25 * 4e-9, C=C, hw=[H, W])
    row("leaky_split planes", reps, lambda: ops.leaky_split(y, 0.2, fp32=False, planes=True), lambda: FC.leaky(y), px * C * 2 * 4e-9, C=C, hw=[H, W])
    row("scale_into 2 flow columns of the fusion input", reps, lambda: ops.scale_into(flow, s, out=buf[:, 134:136]), lambda: flow * s.reshape(-1, 1, 1, 1),
        px * 2 * 2 * 4e-9, hw=[H, W])


def model_rows(pairs, H, W):
    from cremage_amd.pipeline import build_synthetic_film
    m = build_synthetic_film(FC.FULL, device=DEV, seed=FC.SEED)
    sd = {k: v.detach() for k, v in m.state_dict().items()}
    x0, x1 = FC.frames_input("film_time.x0", (1, 3, H, W)).to(DEV), FC.frames_input("film_time.x1", (1, 3, H, W)).to(DEV)
    dt = torch.full((1, 1), 0.5, device=DEV)

    def timed(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        y = fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1), y

    hip = lambda: m(x0, x1, dt)  # noqa: E731
    ref = lambda: FC.interpolator_forward(sd, FC.FULL, x0, x1, dt)["image"][0]  # noqa: E731
    with torch.no_grad():
        for _ in range(2):
            a, b = hip(), ref()
        torch.cuda.synchronize()
        rel = FC.rel_l2(a.cpu(), b.cpu())
        th, tr = [], []
        for _ in range(pairs):
            th.append(timed(hip)[0])
            tr.append(timed(ref)[0])
        out(what="interpolator_call", hw=[H, W], batch=1, params=sum(p.numel() for p in m.parameters()), ms=statistics.median(th), ms_min=min(th),
            ms_all=[round(t, 2) for t in th], torch_ms=statistics.median(tr), torch_ms_min=min(tr), torch_ms_all=[round(t, 2) for t in tr],
            rel_l2_vs_torch=rel, peak_gb=torch.cuda.max_memory_allocated() * 1e-9)
        with ops.profile() as prof:
            hip()
        out(what="interpolator_call_kernels", kernel_ms=sum(f["ms"] for f in prof.result.values()),
            family_ms={k: round(f["ms"], 2) for k, f in sorted(prof.result.items(), key=lambda kv: -kv[1]["ms"]) if f["ms"] > 0},
            slot_ms={k: round(v["ms"], 2) for k, v in sorted(prof.kernels.items(), key=lambda kv: -kv[1]["ms"]) if v["ms"] > 0})


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--pairs", type=int, default=5)
    ap.add_argument("--hw", type=int, nargs=2, default=[576, 1024])
    ap.add_argument("--skip-model", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("film_time: needs the GPU (no timing is taken on a CPU)")
    kernel_rows(a.reps, *a.hw)
    if not a.skip_model:
        model_rows(a.pairs, *a.hw)
