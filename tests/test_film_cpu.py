"""FILM frame interpolation without a GPU: the plain-torch restatement (tests/_film_cases.py) reproduces every `film_*` fixture the
reference wrote, the HIP classes keep the reference's state-dict contract, `pipeline.interpolate_frames` follows the reference's bisecting
schedule and pad / crop geometry, and what is not built raises."""
import hashlib

import pytest
import torch

from cremage_amd import pipeline
from cremage_amd._lib import CrgError
from cremage_amd.film_hip import Interpolator
from cremage_amd.synth import synth_fill_
from tests import _film_cases as FC
from tests.conftest import load_golden

CASES = {"film_tiny": FC.TINY, "film_full": FC.FULL}


def _bound(meta, key):
    """fp32 rounding: 1e-5 relative, or the reference's own fp32-vs-float64 distance where that is larger"""
    return max(1e-5, meta["ref_fp32_vs_fp64"][key])


@pytest.fixture(scope="module")
def models():
    return {tag: synth_fill_(Interpolator(**cfg), FC.SEED, prefix=FC.PREFIX) for tag, cfg in CASES.items()}


@pytest.mark.parametrize("tag", list(CASES))
def test_restatement_reproduces_model_fixture(tag, models):
    meta, arrays = load_golden(tag)
    assert meta["cfg"] == {k: (list(v) if isinstance(v, tuple) else v) for k, v in CASES[tag].items()} and tuple(meta["dts"]) == FC.DTS
    x0, x1, dt = FC.model_inputs(tag, meta["hw"])
    with torch.no_grad():
        out = FC.interpolator_forward(models[tag].state_dict(), CASES[tag], x0, x1, dt)
    assert sorted(f"{k}.{i}" for k, v in out.items() for i in range(len(v))) == sorted(arrays)
    for key, tensors in out.items():
        for i, t in enumerate(tensors):
            name = f"{key}.{i}"
            assert t.shape == arrays[name].shape, name
            err = FC.rel_l2(t, arrays[name])
            assert err <= _bound(meta, name), (name, err, _bound(meta, name))


def test_full_fixture_clamps_at_the_border():
    """the coarsest level is 1 x 2 and the flows exceed it: the border clamp of the warp takes part in the fixture"""
    meta, arrays = load_golden("film_full")
    assert tuple(arrays["forward_residual_flow_pyramid.6"].shape[2:]) == (1, 2)
    assert meta["max_abs_flow"] > 2.0


def test_restatement_reproduces_ops_fixture():
    _, arrays = load_golden("film_ops")
    seen = set()

    def check(name, got):
        seen.add(name)
        assert got.shape == arrays[name].shape, name
        assert FC.rel_l2(got, arrays[name]) <= 1e-5, (name, FC.rel_l2(got, arrays[name]))

    for name, shape, amp, scales in FC.WARP_CASES:
        src, flow = FC.warp_case_inputs(name, shape, amp)
        check(name, FC.warp(src, flow, None if scales is None else torch.tensor(scales)))
    for name, shape in FC.POOL_CASES:
        check(name, FC.avg_pool2(FC.synth(name + ".x", shape)))
    for name, shape in FC.UP_CASES:
        v, res = FC.synth(name + ".v", shape, 3.0), FC.synth(name + ".res", (shape[0], 2, 2 * shape[2], 2 * shape[3]))
        check(name, FC.flow_up2_add(v))
        check(name + "_res", FC.flow_up2_add(v, res))
    for name, cin, cout, k, act in FC.CONV_CASES:
        x, w, b = FC.conv_case_inputs(name, cin, cout, k)
        check(name, FC.conv(x, w, b, act))
        if k == 2:
            check(name + "_up", FC.conv(torch.nn.functional.interpolate(x, scale_factor=2, mode="nearest"), w, b, act))
    assert seen == set(arrays)


def test_float64_truths_agree_with_the_restatement():
    """the float64 formulas the kernel tests use as truth describe the same functions as the fp32 restatement.  Bounds from the
    restatement's arithmetic: its normalised coordinate (|.| <= 9 at flows of +- 2 W) passes through about four fp32 roundings, 2e-6,
    i.e. 7.5e-6 pixels at W = 7, times a slope of at most 2 max|x| per pixel: 1.5e-5 max|x|, asserted with the margin to 1e-4 that still
    separates it from a wrong tap (O(max|x|)); the upsampling is four products and three sums of values <= max|2 v|."""
    for name, shape, amp, scales in FC.WARP_CASES:
        src, flow = FC.warp_case_inputs(name, shape, amp)
        s = None if scales is None else torch.tensor(scales)
        truth = FC.warp_truth(src, flow, s)
        assert (FC.warp(src, flow, s).double() - truth).abs().max() <= 1e-4 * src.abs().max(), name
        zero = torch.zeros_like(flow)
        assert torch.equal(FC.warp_truth(src, zero, s).float(), src), name
    for name, shape in FC.UP_CASES:
        v, res = FC.synth(name + ".v", shape, 3.0), FC.synth(name + ".res", (shape[0], 2, 2 * shape[2], 2 * shape[3]))
        assert (FC.flow_up2_add(v, res).double() - FC.flow_up2_truth(v, res)).abs().max() <= 1e-5 * (2 * v).abs().max(), name


@pytest.mark.parametrize("tag", list(CASES))
def test_state_dict_contract(tag, models):
    meta, _ = load_golden(tag)
    sd = models[tag].state_dict()
    items = sorted(f"{k}:{tuple(v.shape)}" for k, v in sd.items())
    assert len(items) == meta["n_keys"]
    assert hashlib.sha1("\n".join(items).encode()).hexdigest() == meta["keys_sha1"]
    assert sum(p.numel() for p in models[tag].parameters()) == meta["n_params"]
    if tag == "film_full":
        assert meta["n_params"] == FC.FULL_PARAMS
        for key in ("extract.extract_sublevels.convs.0.0.0.weight", "predict_flow._predictor._convs.0.0.weight", "predict_flow._predictors.0._convs.4.0.bias",
                    "fuse.convs.0.0.0.weight", "fuse.output_conv.weight"):
            assert key in sd, key
    fresh = Interpolator(**CASES[tag])
    fresh.load_state_dict(sd, strict=True)


class _StubModel:
    """returns the time of the frame it is asked for, given frames that hold their own time, and records its calls"""
    align = 64

    def __init__(self):
        self.calls = []

    def __call__(self, x0, x1, dt):
        assert x0.shape == x1.shape and x0.shape[0] == 1 and tuple(dt.shape) == (1, 1) and dt.dtype == torch.float32
        self.calls.append((float(x0.flatten()[0]), float(x1.flatten()[0]), float(dt), tuple(x0.shape)))
        return x0 + (x1 - x0) * dt


@pytest.mark.parametrize("n", [1, 2, 3, 7])
def test_schedule_matches_the_reference(n):
    _, arrays = load_golden("film_schedule")
    want = [(int(a), int(b), int(c), d) for a, b, c, d in arrays[f"sched_{n}"].tolist()]
    assert pipeline.film_schedule(n) == want
    model = _StubModel()
    frames = torch.stack([torch.full((3, 64, 64), v) for v in (0.0, 1.0)])
    out = pipeline.interpolate_frames(model, frames, n)
    assert out.shape[0] == n + 2
    assert [(round(a * (n + 1)), round(b * (n + 1)), round((a + (b - a) * dt) * (n + 1)), dt) for a, b, dt, _ in model.calls] == want
    assert torch.allclose(out[:, 0, 0, 0], torch.linspace(0, 1, n + 2), atol=1e-6)


def test_frame_order_and_dropped_frames():
    meta, arrays = load_golden("film_schedule")
    T, n = meta["T"], meta["inter_frames"]
    model = _StubModel()
    frames = torch.stack([torch.full((3, 64, 64), i / (T - 1)) for i in range(T)])
    out = pipeline.interpolate_frames(model, frames, n, as_uint8=True)
    assert out.dtype == torch.uint8 and out.shape[0] == meta["frames"] == (T - 1) * (n + 1) + 1
    assert out[:, 0, 0, 0].tolist() == arrays["order_T3"].tolist()
    assert len(model.calls) == (T - 1) * n


def test_pad_and_crop_geometry():
    """util.pad_batch for a 30 x 50 frame at alignment 64: 34 rows (17 + 17) and 14 columns (7 + 7) of zeros, cropped back"""
    assert pipeline.film_pad_region(30, 50, 64) == ((17, 17, 7, 7), [17, 7, 47, 57])
    assert pipeline.film_pad_region(31, 64, 64) == ((16, 17, 0, 0), [16, 0, 47, 64])
    model = _StubModel()
    frames = torch.stack([torch.full((3, 30, 50), v) for v in (0.25, 0.75)])
    out = pipeline.interpolate_frames(model, frames, 1)
    assert tuple(out.shape) == (3, 3, 30, 50) and torch.equal(out[0], frames[0]) and torch.equal(out[2], frames[1])
    assert all(c[3] == (1, 3, 64, 64) for c in model.calls)
    # signed=True: decode_video's [-1, 1] frames are mapped by clamp((x + 1) / 2, 0, 1) first
    signed = torch.stack([torch.full((3, 30, 50), v) for v in (-1.5, -0.5, 0.5)])
    model = _StubModel()
    out = pipeline.interpolate_frames(model, signed, 1, signed=True)
    assert out[:, 0, 0, 0].tolist() == [0.0, 0.125, 0.25, 0.5, 0.75]
    assert torch.equal(pipeline.interpolate_frames(_StubModel(), ((signed + 1) / 2).clamp(0, 1), 1), out)
    seen = []

    def probe(x0, x1, dt):
        seen.append(x0)
        return x0
    pipeline.interpolate_frames(probe, frames, 1)
    pad = seen[0][0, 0]
    assert float(pad[:17].abs().max()) == 0 and float(pad[47:].abs().max()) == 0 and float(pad[:, :7].abs().max()) == 0 and float(pad[:, 57:].abs().max()) == 0
    assert torch.equal(pad[17:47, 7:57], frames[0, 0])


def test_misaligned_sizes_and_half_precision_raise(models):
    m = models["film_tiny"]
    dt = torch.full((1, 1), 0.5)
    with pytest.raises(CrgError, match="multiples of"):
        m(torch.zeros(1, 3, 24, 48), torch.zeros(1, 3, 24, 48), dt)
    with pytest.raises(CrgError):  # aligned, but a CPU tensor: no fallback
        m(torch.zeros(1, 3, 32, 48), torch.zeros(1, 3, 32, 48), dt)
    with pytest.raises(NotImplementedError):
        Interpolator(**FC.TINY).half()
    with pytest.raises(NotImplementedError):
        Interpolator(**FC.TINY).bfloat16()
    h = Interpolator(**FC.TINY).to(torch.bfloat16)
    with pytest.raises(NotImplementedError):
        h(torch.zeros(1, 3, 32, 48), torch.zeros(1, 3, 32, 48), dt)
    with pytest.raises(NotImplementedError):
        m(torch.zeros(1, 3, 32, 48).half(), torch.zeros(1, 3, 32, 48).half(), dt)
    with pytest.raises(NotImplementedError):
        Interpolator(fusion_pyramid_levels=3)
