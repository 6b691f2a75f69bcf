"""cremage_amd.film_hip.Interpolator on the GPU against what the reference's Interpolator computed on the CPU (`film_tiny` / `film_full`
fixtures: name-keyed synthetic weights, B = 2 with dt = (0.5, 0.25)), and pipeline.interpolate_frames on the real model.

Bounds: every output tensor - the image, every level of both flow pyramids and of both residual flow pyramids - is held to 4 x ITS OWN
rel-L2 measured on the MI355X against the fixture (DESIGN 6 f18 has the table and the command).  The kernels are deterministic; the margin
covers the planner choosing another route for another shape."""
import pytest
import torch

from tests import _film_cases as FC
from tests.conftest import load_golden

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CASES = {"film_tiny": FC.TINY, "film_full": FC.FULL}
# measured rel-L2 of every output tensor against the fixture: [level 0, level 1, ...] per entry of debug_forward
MEASURED = {
    "film_tiny": {"image": [3.199e-06],
                  "forward_residual_flow_pyramid": [1.009e-06, 7.907e-06, 4.294e-06, 3.575e-06, 1.999e-06],
                  "backward_residual_flow_pyramid": [1.114e-06, 7.655e-06, 3.956e-06, 3.489e-06, 1.736e-06],
                  "forward_flow_pyramid": [1.465e-06, 1.520e-06, 1.714e-06, 1.834e-06],
                  "backward_flow_pyramid": [1.573e-06, 1.626e-06, 1.785e-06, 1.889e-06]},
    "film_full": {"image": [6.104e-06],
                  "forward_residual_flow_pyramid": [6.806e-06, 5.184e-06, 9.622e-06, 3.787e-06, 3.659e-06, 3.238e-06, 2.570e-06],
                  "backward_residual_flow_pyramid": [6.653e-06, 5.192e-06, 9.201e-06, 3.496e-06, 3.498e-06, 3.195e-06, 3.431e-06],
                  "forward_flow_pyramid": [1.429e-06, 1.443e-06, 1.475e-06, 1.403e-06, 1.543e-06],
                  "backward_flow_pyramid": [1.474e-06, 1.497e-06, 1.526e-06, 1.449e-06, 1.685e-06]},
}


def bound(tag, key, level):
    return 4.0 * MEASURED[tag][key][level]


@pytest.fixture(scope="module")
def models():
    from cremage_amd import pipeline
    return {tag: pipeline.build_synthetic_film(cfg, device=DEV, seed=FC.SEED) for tag, cfg in CASES.items()}


@pytest.fixture(scope="module")
def runs(models):
    """one B = 2 debug_forward per configuration, shared by the tests below"""
    out = {}
    for tag, m in models.items():
        meta, _ = load_golden(tag)
        x0, x1, dt = (t.to(DEV) for t in FC.model_inputs(tag, meta["hw"]))
        out[tag] = m.debug_forward(x0, x1, dt)
    return out


@pytest.mark.parametrize("tag", list(CASES))
def test_debug_forward_matches_the_reference(tag, runs):
    meta, arrays = load_golden(tag)
    out = runs[tag]
    assert sorted(f"{k}.{i}" for k, v in out.items() for i in range(len(v))) == sorted(arrays)
    worst = {}
    for key, tensors in out.items():
        for i, t in enumerate(tensors):
            name = f"{key}.{i}"
            assert t.shape == arrays[name].shape and t.dtype == torch.float32 and t.is_contiguous() and bool(torch.isfinite(t).all()), name
            err = FC.rel_l2(t.cpu(), arrays[name])
            print(f"[fig] {tag} {name}: rel-L2 {err:.3e}")
            worst[name] = (err, bound(tag, key, i))
    assert all(len(MEASURED[tag][key]) == len(v) for key, v in out.items())
    for name, (err, bnd) in worst.items():
        assert err <= bnd, (name, err, bnd)


@pytest.mark.parametrize("tag", list(CASES))
def test_batch_independence(tag, models, runs):
    """sample 1 of the B = 2 run is the same sample run alone"""
    meta, _ = load_golden(tag)
    x0, x1, dt = (t.to(DEV) for t in FC.model_inputs(tag, meta["hw"]))
    alone = models[tag].debug_forward(x0[1:], x1[1:], dt[1:])
    for key, tensors in runs[tag].items():
        for i, t in enumerate(tensors):
            err = FC.rel_l2(alone[key][i], t[1:])
            print(f"[fig] {tag} {key}.{i}: alone vs in the batch rel-L2 {err:.3e}")
            assert err <= bound(tag, key, i), (key, i, err, bound(tag, key, i))
    assert torch.equal(models[tag](x0[1:], x1[1:], dt[1:]), alone["image"][0])


def test_interpolate_frames(models):
    from cremage_amd import pipeline
    m = models["film_tiny"]
    frames = FC.frames_input("film_frames", (3, 3, 64, 64)).to(DEV)
    n = 3
    video = pipeline.interpolate_frames(m, frames, n)
    assert tuple(video.shape) == (2 * (n + 1) + 1, 3, 64, 64)
    for i in range(3):  # the original frames pass through
        assert torch.equal(video[i * (n + 1)], frames[i])
    sched = pipeline.film_schedule(n)
    for pair in range(2):
        slots = {k: video[pair * (n + 1) + k][None] for k in range(n + 2)}
        for lo, hi, tgt, dt in sched:  # every in-between frame is the direct call the schedule names, on the (clamped) frames it names
            direct = m(slots[lo], slots[hi], torch.full((1, 1), dt, device=DEV)).clamp(0, 1)
            assert torch.equal(direct, slots[tgt]), (pair, lo, hi, tgt, dt)
    u8 = pipeline.interpolate_frames(m, frames, n, as_uint8=True)
    assert u8.dtype == torch.uint8 and torch.equal(u8, (video * 255).byte())
    # a size that needs the pad: 40 x 56 at the tiny configuration's alignment of 16 -> 48 x 64 inside, 40 x 56 outside
    small = frames[:2, :, :40, :56].contiguous()
    out = pipeline.interpolate_frames(m, small, 1)
    assert tuple(out.shape) == (3, 3, 40, 56) and torch.equal(out[0], small[0]) and torch.equal(out[2], small[1])
    (top, bottom, left, right), _ = pipeline.film_pad_region(40, 56, m.align)
    padded = torch.nn.functional.pad(small, (left, right, top, bottom))
    mid = m(padded[0:1], padded[1:2], torch.full((1, 1), 0.5, device=DEV)).clamp(0, 1)[:, :, top:top + 40, left:left + 56]
    assert torch.equal(out[1:2], mid)
