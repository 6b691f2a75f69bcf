"""Device time and parity of the face unblur / colorize network (cremage_amd.unblur_hip, fp32 class), one face of 256 x 256 at batch 1:

  * each of the network's eight transposed-conv shapes, `ops.conv_transpose2d` against the composed form made of the kernels that existed
    before it (tests/_unblur_cases.py: the 2 x 2 taps of each parity embedded in a zero 3 x 3 kernel, 4 Cout output channels, pixel
    shuffle), both replayed from a captured hipGraph (median and minimum of the replays, random data), with the weight bytes the new
    route has to read over its time;
  * `ops.group_norm_add_act` against ops.group_norm + add + F.silu + ops.split_bf16 at the block tails of three levels;
  * one model call in three arms, in alternating triples inside one process (device events around each call, all warmed up): this path,
    the plain-torch restatement on PyTorch-ROCm fp32, and this path inside `composed_arm` - plus this path's device time per kernel family;
  * --parity: rel-L2 of the composed arm and of this path against every fixture of tests/golden/unblur_*.npz, per tensor - the figures
    the bounds of tests/test_unblur_models_gpu.py are made of;
  * --glue: pipeline.unblur_faces on one face of a 512 x 512 and of a 1024 x 1024 image, glue "host" against glue "device" in alternating
    triples (host clock around a call that ends in a device synchronise; median), with the model call taken off and, as a direct
    reading of the glue, with an identity model; the two glue kernels alone, replayed from a captured graph; and the eager model call
    against its hipGraph replay (graph=True), alternating, with what the graph's memory pool holds.  These rows take the place of the
    three-arm model rows.

    python tools/unblur_time.py [--reps 20] [--triples 5] [--parity] [--glue] [--skip-model] [--skip-kernels]
Prints one JSON line per measurement.  Nothing is asserted."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from cremage_amd import ops  # noqa: E402
from tests import _unblur_cases as UC  # noqa: E402
from tests.conftest import load_golden  # noqa: E402
from tools.svd_time import graph_ms  # noqa: E402

DEV = "cuda:0"


def out(**kw):
    print(json.dumps(kw), flush=True)


def cl(n, c, h, w, scale=1.0):
    return (torch.randn(n, h, w, c, device=DEV) * scale).permute(0, 3, 1, 2)


def convt_rows(reps):
    for cin, cout, side in UC.CONVT_MODEL_SHAPES:
        x = cl(1, cin, side, side)
        w = torch.randn(cin, cout, 4, 4, device=DEV) * (16 * cin) ** -0.5
        hi, lo = ops.split_bf16(x)
        w3, _ = UC.composed_convt_weight(w)
        new = lambda: ops.conv_transpose2d(hi, lo, w)  # noqa: E731
        conv = lambda: ops.conv2d(hi, w3, None, padding=1, x_lo=lo)  # noqa: E731  (the composed form without its pixel shuffle)

        def comp():
            y = conv()
            return y.reshape(1, 2, 2, cout, side, side).permute(0, 3, 4, 1, 5, 2).reshape(1, cout, 2 * side, 2 * side).contiguous(memory_format=torch.channels_last)
        new()
        route = ops.last_route()
        a, b, c = graph_ms(new, reps), graph_ms(comp, reps), graph_ms(conv, reps)
        live = (2 if side > 1 else 1) ** 2
        wbytes = 4.0 * 4 * live * cin * cout  # hi + lo planes of the taps walked
        out(what="conv_transpose2d", cin=cin, cout=cout, grid=[side, side], ms=a[0], ms_min=a[1], composed_ms=b[0], composed_ms_min=b[1], composed_conv_only_ms=c[0],
            weight_gb_per_s=wbytes / a[0] * 1e-6, tile=[32 * route["config"], 32 * route["wnt"]])
        del w3


def gn_rows(reps):
    import torch.nn.functional as F
    for c, groups, side in ((64, 32, 128), (320, 32, 16), (1024, 32, 2)):
        x, sk = cl(1, c, side, side), cl(1, c, side, side)
        g, b = torch.ones(c, device=DEV), torch.zeros(c, device=DEV)
        new = lambda: ops.group_norm_add_act(x, g, b, groups, 1e-5, skip=sk, planes=True)  # noqa: E731
        comp = lambda: UC.composed_gn_add_act(x, g, b, groups, 1e-5, sk, True)  # noqa: E731
        a, bb = graph_ms(new, reps), graph_ms(comp, reps)
        gb = x.numel() * (4 + 4 + 4 + 4) * 1e-9  # x, skip in; y and the two planes out
        out(what="group_norm_add_act", c=c, groups=groups, grid=[side, side], ms=a[0], ms_min=a[1], gb_per_s=gb / a[0] * 1e3, composed_ms=bb[0], composed_ms_min=bb[1])


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    y = fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1), y


def model_rows(triples, m):
    sd = {k: v.detach() for k, v in m.state_dict().items()}
    x = UC.full_input(1).to(DEV)
    hip = lambda: m(x)  # noqa: E731
    ref = lambda: UC.model_forward(x, sd)[0]  # noqa: E731

    def comp():
        with UC.composed_arm():
            return m(x)
    with torch.no_grad():
        for _ in range(2):
            a, b, c = hip(), ref(), comp()
        torch.cuda.synchronize()
        th, tr, tc = [], [], []
        for _ in range(triples):
            th.append(timed(hip)[0])
            tr.append(timed(ref)[0])
            tc.append(timed(comp)[0])
        out(what="model_call", hw=list(UC.FULL_HW), batch=1, params=sum(p.numel() for p in m.parameters()), ms=statistics.median(th), ms_min=min(th),
            ms_all=[round(t, 2) for t in th], torch_ms=statistics.median(tr), torch_ms_min=min(tr), torch_ms_all=[round(t, 2) for t in tr],
            composed_ms=statistics.median(tc), composed_ms_min=min(tc), composed_ms_all=[round(t, 2) for t in tc],
            rel_l2_vs_torch=UC.rel_l2(a, b), rel_l2_composed_vs_torch=UC.rel_l2(c, b), peak_gb=torch.cuda.max_memory_allocated() * 1e-9)
        with ops.profile() as prof:
            hip()
        out(what="model_call_kernels", kernel_ms=sum(f["ms"] for f in prof.result.values()),
            family_ms={k: round(f["ms"], 3) for k, f in sorted(prof.result.items(), key=lambda kv: -kv[1]["ms"]) if f["ms"] > 0},
            slot_ms={k: round(v["ms"], 3) for k, v in sorted(prof.kernels.items(), key=lambda kv: -kv[1]["ms"]) if v["ms"] > 0})


def parity_rows(m):
    """composed arm and this path against the reference's own outputs, per fixture tensor"""
    with torch.no_grad():
        for name in UC.BLOCK_CASES:
            meta, arrays = load_golden("unblur_" + name)
            blk = UC.build_block(name, DEV)
            x = UC.block_input(name).to(DEV)
            y = UC.run_block(blk, x)
            with UC.composed_arm():
                yc = UC.run_block(blk, x)
            out(what="parity", fixture=name, tensor="y", new=UC.rel_l2(y, arrays["y"]), composed=UC.rel_l2(yc, arrays["y"]), ref_own=meta["ref_fp32_vs_fp64"]["y"])
        if m is None:
            return
        meta, arrays = load_golden("unblur_full")
        x = UC.full_input(meta["batch"]).to(DEV)
        got = UC.full_tensors(m.debug_forward(x))
        with UC.composed_arm():
            gotc = UC.full_tensors(m.debug_forward(x))
        for k in sorted(arrays):
            out(what="parity", fixture="full", tensor=k, new=UC.rel_l2(UC.sampled(got[k]), arrays[k]), composed=UC.rel_l2(UC.sampled(gotc[k]), arrays[k]),
                ref_own=meta["ref_fp32_vs_fp64"][k])


def wall(fn):
    """milliseconds of fn on the host clock, the device drained before and after"""
    import time
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    y = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, y


class _Identity(torch.nn.Module):
    """a model that costs nothing: what is left of an arm is its glue"""

    def __init__(self):
        super().__init__()
        self.one = torch.nn.Parameter(torch.ones(()))

    def forward(self, x):
        return x


def glue_rows(triples, reps, m):
    import numpy as np
    from cremage_amd import pipeline, postprocess as PP
    ident = _Identity().to(DEV)
    tpl = np.array(PP.UNBLUR_LANDMARKS_256)
    with torch.no_grad():
        x = UC.full_input(1).to(DEV)
        for _ in range(2):
            m(x)
        model_ms = statistics.median(wall(lambda: m(x))[0] for _ in range(max(triples, 3)))
        for side in (512, 1024):
            img = np.random.RandomState(side).randint(1, 256, size=(side, side, 3)).astype(np.uint8)
            lms = [tpl * (side / 640.0) + [side * 0.3, side * 0.25]]  # a face of 0.4 of the image's side
            mat = PP.similarity_from_landmarks(lms[0])
            row = dict(what="glue", image=[side, side], faces=1, model_call_ms=model_ms, footprint=list(PP.warped_footprint(mat, (256, 256), (side, side))))
            for name, model in (("", m), ("identity_", ident)):
                host = lambda: pipeline.unblur_faces(model, img, lms, glue="host")  # noqa: E731
                dev = lambda: pipeline.unblur_faces(model, img, lms, glue="device")  # noqa: E731
                a, b = host(), dev()
                row[name + "equal"] = bool(np.array_equal(a, b.cpu().numpy()))
                th, td = [], []
                for _ in range(triples):
                    th.append(wall(host)[0])
                    td.append(wall(dev)[0])
                row.update({name + "host_ms": statistics.median(th), name + "host_ms_all": [round(t, 2) for t in th],
                            name + "device_ms": statistics.median(td), name + "device_ms_all": [round(t, 2) for t in td]})
            row["host_outside_model_ms"] = row["host_ms"] - model_ms
            row["device_outside_model_ms"] = row["device_ms"] - model_ms
            # the two kernels alone, replayed from a graph: the coefficients are kernel arguments, so they are captured
            imgd = torch.from_numpy(img).to(DEV)
            face = torch.rand(1, 3, 256, 256, device=DEV).contiguous(memory_format=torch.channels_last)
            xin = ops.empty_image(1, 3, 256, 256, torch.float32, DEV)
            inv = PP.invert_affine(mat)
            rect = PP.warped_footprint(mat, (256, 256), (side, side))
            w = graph_ms(lambda: ops.warp_affine_u8(imgd, inv[None], (256, 256), out=xin), reps)
            p = graph_ms(lambda: ops.paste_warped_u8(imgd, face, mat, rect=rect), reps)
            pw = graph_ms(lambda: ops.paste_warped_u8(imgd, face, mat, rect=(0, 0, side, side)), reps)
            row.update(warp_kernel_ms=w[0], warp_kernel_ms_min=w[1], paste_kernel_ms=p[0], paste_kernel_ms_min=p[1], paste_whole_image_ms=pw[0])
            out(**row)
        # eager call against graph replay, alternating
        torch.cuda.synchronize()
        base, base_res = torch.cuda.memory_allocated(), torch.cuda.memory_reserved()
        g = pipeline._graphed_unblur(m)
        g(x)
        torch.cuda.synchronize()
        pool, pool_res = torch.cuda.memory_allocated() - base, torch.cuda.memory_reserved() - base_res
        same = bool(torch.equal(g(x), m(x)))
        te, tg = [], []
        for _ in range(max(triples, 3)):
            te.append(wall(lambda: m(x))[0])
            tg.append(wall(lambda: g(x))[0])
        out(what="model_call_graph", eager_ms=statistics.median(te), eager_ms_all=[round(t, 2) for t in te], replay_ms=statistics.median(tg),
            replay_ms_all=[round(t, 2) for t in tg], equal=same, captures=g.captures, replays=g.replays, graph_held_gb=pool * 1e-9, graph_reserved_gb=pool_res * 1e-9,
            peak_gb=torch.cuda.max_memory_allocated() * 1e-9)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--triples", type=int, default=5)
    ap.add_argument("--parity", action="store_true")
    ap.add_argument("--glue", action="store_true")
    ap.add_argument("--skip-model", action="store_true")
    ap.add_argument("--skip-kernels", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("unblur_time: needs the GPU (no timing is taken on a CPU)")
    if not a.skip_kernels:
        convt_rows(a.reps)
        gn_rows(a.reps)
    model = None
    if not a.skip_model:
        from cremage_amd.pipeline import build_synthetic_unblur
        model = build_synthetic_unblur(DEV, UC.SEED)
    if a.parity:
        parity_rows(model)
    if model is not None and a.glue:
        glue_rows(a.triples, a.reps, model)
    elif model is not None:
        model_rows(a.triples, model)
