"""Timing and parity of ControlNet's HED annotator on the device.

    python tools/hed_time.py [--rounds 3] [--reps 10] [--json PATH]     three arms at 512 x 512 and 768 x 512, alternating inside one call
    python tools/hed_time.py --parity [--json PATH]                      rel-L2 of the composed arm (and of the new path) per fixture tensor

Arms: "torch" - the functional restatement of tests/_hed_cases.py in PyTorch fp32 on the device; "composed" - cremage_amd.annotator_hip
with ops.relu_pool_proj replaced by what existed before it (tests/_hed_cases.composed_arm); "new" - cremage_amd.annotator_hip as it is.
Every arm is warmed up at every size first; a round times `reps` forwards per arm between two device events, the arms taking turns; the
figure of an arm is the median over the rounds, the spread is printed next to it.  Then the new path's time per launch family
(ops.profile, eager, one forward) and the glue from the resized bytes to the edge map: host arm (download the five projections,
postprocess.hed_fuse_host) against device arm (ops.hed_fuse), network included and tail alone.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from cremage_amd import annotator_hip, ops  # noqa: E402
from cremage_amd import postprocess as PP  # noqa: E402
from tests import _hed_cases as HC  # noqa: E402

DEV = "cuda"
SIZES = ((512, 512), (768, 512))  # (H, W)
GOLD = os.path.join(REPO, "tests", "golden")


def _events_ms(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def _host_ms(fn, reps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3 / reps


def timing(rounds, reps):
    model = HC.build_full(DEV)
    sd = {k: v.detach() for k, v in model.state_dict().items()}
    out = {}
    for hw in SIZES:
        x = HC.image_input(f"time.{hw[0]}x{hw[1]}", (1, 3) + hw).to(DEV)

        def arm_torch():
            with torch.no_grad():
                return HC.hed_forward(x, sd)

        def arm_composed():
            with HC.composed_arm():
                return model(x)

        def arm_new():
            return model(x)

        arms = {"torch": arm_torch, "composed": arm_composed, "new": arm_new}
        for fn in arms.values():  # warm-up: code objects, packed weights, torch's conv algorithm choice
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        ms = {k: [] for k in arms}
        for _ in range(rounds):
            for k, fn in arms.items():
                ms[k].append(_events_ms(fn, reps))
        res = {k: dict(median_ms=statistics.median(v), min_ms=min(v), max_ms=max(v)) for k, v in ms.items()}
        with ops.profile() as prof:
            arm_new()
        res["new_by_family"] = {k: dict(ms=v["ms"], launches=v["launches"]) for k, v in prof.result.items() if v["launches"]}
        res["new_by_kernel"] = {k: dict(ms=v["ms"], launches=v["launches"]) for k, v in prof.kernels.items() if v["launches"]}
        # the glue: resized bytes -> edge map
        img = HC.image_input(f"time.img.{hw[0]}x{hw[1]}", hw + (3,)).to(torch.uint8).numpy()
        det = annotator_hip.HEDdetector(model)
        for g in ("host", "device"):
            det(img, glue=g)
        projs = det.projections(img)
        torch.cuda.synchronize()

        def tail_host():
            return PP.hed_fuse_host([e.detach().cpu().numpy().astype(np.float32)[0, 0] for e in projs], hw)

        def tail_device():
            return ops.hed_fuse(projs, hw)

        glue = {k: [] for k in ("host", "device", "tail_host", "tail_device")}
        for _ in range(rounds):
            glue["host"].append(_host_ms(lambda: det(img, glue="host"), reps))
            glue["device"].append(_host_ms(lambda: det(img, glue="device"), reps))
            glue["tail_host"].append(_host_ms(tail_host, reps))
            glue["tail_device"].append(_host_ms(tail_device, reps))
        res["glue_ms"] = {k: dict(median_ms=statistics.median(v), min_ms=min(v), max_ms=max(v)) for k, v in glue.items()}
        same = bool(np.array_equal(det(img, glue="host"), det(img, glue="device").cpu().numpy()))
        res["glue_bytes_equal"] = same
        out[f"{hw[0]}x{hw[1]}"] = res
        print(f"== {hw[0]} x {hw[1]}  (ms per forward, median of {rounds} rounds x {reps} reps [min .. max])")
        for k in arms:
            r = res[k]
            print(f"   {k:9s} {r['median_ms']:8.3f}  [{r['min_ms']:.3f} .. {r['max_ms']:.3f}]")
        for k, v in sorted(res["new_by_family"].items(), key=lambda kv: -kv[1]["ms"]):
            print(f"   new / {k:14s} {v['ms']:8.3f} ms  {v['launches']} launches")
        for k, v in sorted(res["new_by_kernel"].items(), key=lambda kv: -kv[1]["ms"]):
            print(f"   new kernel {k:22s} {v['ms']:8.3f} ms  {v['launches']} launches")
        for k, r in res["glue_ms"].items():
            print(f"   glue {k:12s} {r['median_ms']:8.3f}  [{r['min_ms']:.3f} .. {r['max_ms']:.3f}]")
        print(f"   glue bytes equal: {same}")
    return out


def _fixture(name):
    z = np.load(os.path.join(GOLD, name + ".npz"))
    return z, json.loads(str(z["meta"]))


def parity():
    """rel-L2 against the fixtures, per tensor: {'composed': {...}, 'new': {...}}"""
    out = {"composed": {}, "new": {}}
    for name, (_, _, down) in HC.BLOCK_CASES.items():
        z, _ = _fixture("hed_" + name)
        m = HC.build_block(name, DEV)
        x = HC.block_input(name).to(DEV)
        for arm in ("composed", "new"):
            if arm == "composed":
                with HC.composed_arm():
                    h, proj = m(x, down_sampling=down)
            else:
                h, proj = m(x, down_sampling=down)
            out[arm][name] = dict(h=HC.rel_l2(h, torch.from_numpy(z["h"])), proj=HC.rel_l2(proj, torch.from_numpy(z["proj"])))
    model = HC.build_full(DEV)
    for name in HC.FULL_CASES:
        z, _ = _fixture("hed_" + name)
        x = HC.full_input(name).to(DEV)
        for arm in ("composed", "new"):
            if arm == "composed":
                with HC.composed_arm():
                    got = model(x)
            else:
                got = model(x)
            out[arm][name] = {f"proj{i + 1}": HC.rel_l2(p, torch.from_numpy(z[f"proj{i + 1}"])) for i, p in enumerate(got)}
    for arm in out:
        print(f"== {arm} arm, rel-L2 against the fixtures")
        for name, d in out[arm].items():
            print(f"   {name:22s} " + "  ".join(f"{k} {v:.3e}" for k, v in d.items()))
    print("COMPOSED_REL_L2 = " + json.dumps(out["composed"]))
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--parity", action="store_true")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("hed_time: no HIP device - a timing or a parity figure needs the GPU")
    if a.rounds < 3:
        raise SystemExit("hed_time: at least three rounds")
    with torch.no_grad():
        result = parity() if a.parity else timing(a.rounds, a.reps)
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(result, f, indent=1)
