"""ORACLE tooling for FILM frame interpolation - writes tests/golden/film_*.npz from the reference's own modules
(modules/frame_interpolation_pytorch: Interpolator, util.warp / Conv2d, inference_multiple_frames._interpolate_two_frames) on the name-keyed
synthetic weights and `synth_input` tensors, with the import stubs of oracle/gen_golden.py (imported, not changed) plus a stand-in for
`cv2`, which the reference imports for file I/O only.  Only outputs and metadata are stored; shapes and inputs are those of
tests/_film_cases.py.  A rerun reproduces the fixtures exactly (apart from timing meta).

    python tools/gen_golden_film.py [--only NAME ...]
"""
import argparse
import hashlib
import os
import sys
import time
import types

import numpy as np
import torch
import torch.nn.functional as F

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from oracle import gen_golden as G  # noqa: E402,F401  (installs the import stubs and puts the reference on sys.path)
from oracle.gen_golden import SEED, save, synth_fill_  # noqa: E402
from tests import _film_cases as FC  # noqa: E402

assert SEED == FC.SEED


def _modules():
    if "cv2" not in sys.modules:
        sys.modules["cv2"] = types.ModuleType("cv2")  # file I/O only (util.load_image, the mp4 writer): never called here
    from frame_interpolation_pytorch import inference_multiple_frames, interpolator, util
    return interpolator, util, inference_multiple_frames


def _key_digest(module):
    items = sorted(f"{k}:{tuple(v.shape)}" for k, v in module.state_dict().items())
    return hashlib.sha1("\n".join(items).encode()).hexdigest(), len(items)


def _rel(a, b):
    return float((a.double() - b).norm() / b.norm().clamp_min(1e-30))


def _model_case(tag, cfg, hw):
    I, _, _ = _modules()
    m = I.Interpolator(**cfg)
    synth_fill_(m, SEED, prefix=FC.PREFIX)
    m.eval()
    x0, x1, dt = FC.model_inputs(tag, hw)
    t0 = time.time()
    with torch.no_grad():
        out = m.debug_forward(x0, x1, dt)
        secs = time.time() - t0
        out64 = m.double().debug_forward(x0.double(), x1.double(), dt.double())  # the reference's own fp32 rounding, per output
        m.float()
    arrays, own = {}, {}
    for key, tensors in out.items():
        for i, t in enumerate(tensors):
            arrays[f"{key}.{i}"] = t
            own[f"{key}.{i}"] = _rel(t, out64[key][i])
    sha, n = _key_digest(m)
    save(tag, dict(cfg={k: (list(v) if isinstance(v, tuple) else v) for k, v in cfg.items()}, hw=list(hw), dts=list(FC.DTS), seed=SEED, prefix=FC.PREFIX,
                   n_params=sum(p.numel() for p in m.parameters()), n_keys=n, keys_sha1=sha, ref_fp32_vs_fp64=own,
                   max_abs_flow=float(max(t.abs().max() for t in out["forward_flow_pyramid"] + out["backward_flow_pyramid"])),
                   ref_cpu_seconds=secs, threads=torch.get_num_threads()), **arrays)


def g_tiny():
    _model_case("film_tiny", FC.TINY, (32, 48))


def g_full():
    _model_case("film_full", FC.FULL, (64, 128))


def g_ops():
    _, U, _ = _modules()
    arrays = {}
    with torch.no_grad():
        for name, shape, amp, scales in FC.WARP_CASES:
            src, flow = FC.warp_case_inputs(name, shape, amp)
            if scales is not None:  # multiply_pyramid, then util.warp
                flow = U.multiply_pyramid([flow], torch.tensor(scales, dtype=torch.float32).reshape(-1, 1))[0]
            arrays[name] = U.warp(src, flow)
        for name, shape in FC.POOL_CASES:
            arrays[name] = F.avg_pool2d(FC.synth(name + ".x", shape), 2, 2)
        for name, shape in FC.UP_CASES:
            v = FC.synth(name + ".v", shape, 3.0)
            res = FC.synth(name + ".res", (shape[0], 2, 2 * shape[2], 2 * shape[3]))
            up = F.interpolate(2 * v, size=res.shape[2:4], mode="bilinear")  # pyramid_flow_estimator.py:134, util.py:115
            arrays[name] = up
            arrays[name + "_res"] = res + up
        for name, cin, cout, k, act in FC.CONV_CASES:
            m = U.Conv2d(cin, cout, size=k, activation="relu" if act else None)
            synth_fill_(m, SEED, prefix="film_ops." + name + ".")
            x, w, b = FC.conv_case_inputs(name, cin, cout, k)
            assert torch.equal(w, m[0].weight) and torch.equal(b, m[0].bias)
            arrays[name] = m(x)
            if k == 2:  # behind the fusion's nearest x 2 (fusion.py:120-121)
                arrays[name + "_up"] = m(F.interpolate(x, size=(2 * x.shape[2], 2 * x.shape[3]), mode="nearest"))
    save("film_ops", dict(seed=SEED, conv_hw=list(FC.CONV_HW)), **arrays)


def g_schedule():
    """_interpolate_two_frames with a stub model and a stubbed load_image: frame k of a clip is the constant image k / (T - 1); the
    stub model returns x0 + (x1 - x0) * dt, the time of the frame it is asked for, so every call tells its two sources and its target."""
    _, _, M = _modules()
    arrays, meta = {}, {}
    hw, calls = (4, 6), []

    def load_image(path, align=64):
        return np.full((1,) + hw + (3,), np.float32(path), dtype=np.float32), [0, 0, hw[0], hw[1]]

    def model(x0, x1, dt):
        calls.append((float(x0.flatten()[0]), float(x1.flatten()[0]), float(dt)))
        return x0 + (x1 - x0) * dt

    M.load_image = load_image
    for n in (1, 2, 3, 7):
        del calls[:]
        frames = M._interpolate_two_frames(0.0, 1.0, n, False, False, model, False)
        assert len(frames) == n + 2
        sched = [(round(a * (n + 1)), round(b * (n + 1)), round((a + (b - a) * dt) * (n + 1)), dt) for a, b, dt in calls]
        arrays[f"sched_{n}"] = np.array(sched, dtype=np.float64)
    T, n = 3, 3
    out = []
    for i in range(1, T):  # inference_multiple_frames:53-64
        out.append(M._interpolate_two_frames((i - 1) / (T - 1), i / (T - 1), n, False, False, model, i != 1))
    video = np.concatenate(out, axis=0)
    arrays["order_T3"] = video[:, 0, 0, 0].astype(np.uint8)
    meta.update(T=T, inter_frames=n, frames=int(video.shape[0]))
    save("film_schedule", meta, **arrays)


ALL = dict(tiny=g_tiny, full=g_full, ops=g_ops, schedule=g_schedule)

if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", nargs="*", default=None)
    a = ap.parse_args()
    torch.manual_seed(0)
    for key, fn in ALL.items():
        if a.only and key not in a.only:
            continue
        fn()
