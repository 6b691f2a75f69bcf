"""The host side of the ControlNet annotators (cremage_amd.postprocess: hwc3, annotator_size, hed_fuse_host, nms_host,
fake_scribble_from_hed, scribble_map) on hand cases, the margin condition that makes the GPU byte comparisons strict, and the fixtures'
key contract.  No GPU."""
import json
import os

import numpy as np
import pytest
import torch

from cremage_amd import postprocess as PP
from tests import _hed_cases as HC

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _load(name):
    z = np.load(os.path.join(GOLD, name + ".npz"))
    return z, json.loads(str(z["meta"]))


# ---- hwc3 / annotator_size / scribble_map ------------------------------------------------------------------------------------------------------
def test_hwc3_hand_cases():
    g = np.array([[0, 7], [200, 255]], dtype=np.uint8)
    assert np.array_equal(PP.hwc3(g), np.stack([g, g, g], axis=2))
    assert np.array_equal(PP.hwc3(g[:, :, None]), np.stack([g, g, g], axis=2))
    rgb = np.arange(12, dtype=np.uint8).reshape(2, 2, 3)
    assert PP.hwc3(rgb) is rgb
    rgba = np.array([[[100, 50, 0, 255], [100, 50, 0, 0]], [[100, 50, 0, 51], [10, 20, 30, 128]]], dtype=np.uint8)
    # alpha 255: the colour; alpha 0: white; alpha 51 = 0.2: 0.2 c + 204; alpha 128: truncation of c * a + 255 (1 - a) in float32
    a = np.float32(128) / np.float32(255.0)
    want = np.array([[[100, 50, 0], [255, 255, 255]], [[224, 214, 204], [int(np.float32(c) * a + np.float32(255.0) * (np.float32(1.0) - a)) for c in (10, 20, 30)]]],
                    dtype=np.uint8)
    assert np.array_equal(PP.hwc3(rgba), want)
    with pytest.raises(ValueError):
        PP.hwc3(np.zeros((2, 2, 2), dtype=np.uint8))
    with pytest.raises(ValueError):
        PP.hwc3(np.zeros((2, 2, 3), dtype=np.float32))


@pytest.mark.parametrize("h, w, res, want", [
    (512, 768, 512, (512, 768)),      # k = 1: already multiples of 64
    (95, 95, 95, (64, 64)),           # 95 / 64 = 1.48 -> 1
    (96, 96, 96, (128, 128)),         # 96 / 64 = 1.5: half to even -> 2
    (160, 160, 160, (128, 128)),      # 2.5: half to even -> 2 (round-half-up would give 192)
    (224, 224, 224, (256, 256)),      # 3.5 -> 4
    (96, 160, 64, (64, 128)),         # k = 2 / 3 < 1: 64 x 106.67 -> 1.67 -> 2
    (100, 50, 100, (192, 128)),       # k = 2 > 1: 200 x 100 -> 3.125 -> 3, 1.5625 -> 2
])
def test_annotator_size(h, w, res, want):
    H, W, k = PP.annotator_size(h, w, res)
    assert (H, W) == want
    assert k == float(res) / min(h, w)


def test_resize_for_annotator_filters_and_identity():
    img = (np.arange(96 * 160 * 3) % 251).astype(np.uint8).reshape(96, 160, 3)
    out = PP.resize_for_annotator(img, 64)  # k < 1: BOX
    assert out.shape == (64, 128, 3) and out.dtype == np.uint8
    same = np.zeros((64, 128, 3), dtype=np.uint8)
    assert PP.resize_for_annotator(same, 64) is same
    up = PP.resize_for_annotator(np.full((50, 100, 3), 9, dtype=np.uint8), 100)  # k = 2 > 1: LANCZOS, a constant stays constant
    assert up.shape == (128, 192, 3) and (up == 9).all()
    with pytest.raises(ValueError):
        PP.resize_for_annotator(np.zeros((10, 400, 3), dtype=np.uint8), 10)  # the short edge rounds to 0


def test_scribble_map():
    img = np.array([[[126, 200, 200], [127, 127, 127]], [[255, 255, 0], [200, 130, 128]]], dtype=np.uint8)
    want = np.array([[[255] * 3, [0] * 3], [[255] * 3, [0] * 3]], dtype=np.uint8)
    assert np.array_equal(PP.scribble_map(img), want)


# ---- hed_fuse_host -----------------------------------------------------------------------------------------------------------------------------
def test_hed_tables_hand_case():
    # 2 -> 4: scale 0.5; f = (d + 0.5) / 2 - 0.5 = -0.25, 0.25, 0.75, 1.25 -> (0, 0), (0, 0.25), (0, 0.75), s = 1 >= in - 1 -> (1, 0)
    s, f = PP.hed_tables(2, 4)
    assert s.tolist() == [0, 0, 0, 1] and f.tolist() == [0.0, 0.25, 0.75, 0.0]
    assert s.dtype == np.int32 and f.dtype == np.float32
    s, f = PP.hed_tables(1, 5)
    assert s.tolist() == [0] * 5 and f.tolist() == [0.0] * 5
    s, f = PP.hed_tables(7, 7)
    assert s.tolist() == [0, 1, 2, 3, 4, 5, 6] and f.tolist() == [0.0] * 7


def test_hed_fuse_constant_same_size_and_broadcast():
    c = np.full((3, 5), 0.75, dtype=np.float32)
    e, mean = PP.hed_fuse_host([c, np.full((2, 2), 0.75, dtype=np.float32), np.full((1, 1), 0.75, dtype=np.float32)], (3, 5), return_logit=True)
    assert (mean == np.float32(0.75)).all() and len(np.unique(e)) == 1
    m = (np.arange(15, dtype=np.float32).reshape(3, 5) - 7) / 3
    e, mean = PP.hed_fuse_host([m], (3, 5), return_logit=True)
    assert np.array_equal(mean, m) and mean is not m  # already at the size: copied, untouched
    one = np.array([[1.5]], dtype=np.float32)
    e, mean = PP.hed_fuse_host([one], (4, 6), return_logit=True)
    assert mean.shape == (4, 6) and (mean == np.float32(1.5)).all()
    small = m[:2, :3].copy()
    batched = PP.hed_fuse_host([np.stack([small, -small])], (3, 5))  # a batch is its samples, one by one
    assert batched.shape == (2, 3, 5)
    assert np.array_equal(batched[0], PP.hed_fuse_host([small], (3, 5))) and np.array_equal(batched[1], PP.hed_fuse_host([-small], (3, 5)))


def test_hed_fuse_2x2_to_4x4_by_hand():
    m = np.array([[0.0, 4.0], [8.0, 12.0]], dtype=np.float32)
    # per axis the weights of the second sample are 0, 0.25, 0.75, 1 (test_hed_tables_hand_case): rows 0, 1, 3, 4 / 8, 9, 11, 12, then
    # the same weights between the two rows
    want = np.array([[0, 1, 3, 4], [2, 3, 5, 6], [6, 7, 9, 10], [8, 9, 11, 12]], dtype=np.float32)
    _, mean = PP.hed_fuse_host([m], (4, 4), return_logit=True)
    assert np.array_equal(mean, want)
    _, mean = PP.hed_fuse_host([m, want], (4, 4), return_logit=True)  # (u1 + u2) / 2
    assert np.array_equal(mean, want)


def test_hed_fuse_byte_truncation():
    # logit 0: e = 0.5, 127.5 -> 127 (truncation, not rounding); ln 3: e = 0.75, 191.25 -> 191; 2: e * 255 = 224.6 -> 224;
    # 40: 1 + exp(-40) is 1 in double, e = 1 -> 255; -40: e = 4e-18 -> 0
    m = np.array([[0.0, np.log(3.0), 2.0, 40.0, -40.0]], dtype=np.float32)
    e = PP.hed_fuse_host([m], (1, 5))
    assert e.dtype == np.uint8 and e.tolist() == [[127, 191, 224, 255, 0]]


def _margin(mean):
    v = (1.0 / (1.0 + np.exp(-mean.astype(np.float64)))) * 255.0
    return float(np.abs(v - np.rint(v)).min())


@pytest.mark.parametrize("name", sorted(HC.FUSE_CASES))
def test_margin_of_the_fuse_cases(name):
    """the GPU byte comparison of this case is strict only if no e * 255 lies next to an integer: a last-place difference between two
    exp's moves the value by about 1e-13; the excluded set must be EMPTY (a violating case gets another seed, never a tolerance)"""
    maps = [m.numpy() for m in HC.fuse_maps(name)]
    _, mean = PP.hed_fuse_host(maps, HC.FUSE_CASES[name][0], return_logit=True)
    d = _margin(mean)
    print(name, "min distance of e * 255 to an integer:", d)
    assert d > HC.MARGIN


@pytest.mark.parametrize("name", sorted(HC.FULL_CASES))
def test_margin_of_the_full_fixtures(name):
    z, meta = _load("hed_" + name)
    maps = [z[f"proj{i}"][:, 0] for i in range(1, 6)]
    _, mean = PP.hed_fuse_host(maps, tuple(meta["hw"]), return_logit=True)
    d = _margin(mean)
    print(name, "min distance of e * 255 to an integer:", d, "logits", float(mean.min()), float(mean.max()))
    assert d > HC.MARGIN


# ---- nms / fake scribble -------------------------------------------------------------------------------------------------------------------------
def test_nms_isolated_ridge_survives():
    x = np.zeros((31, 31), dtype=np.uint8)
    x[:, 15] = 255  # a vertical ridge: after the blur every pixel of column 15 is the maximum of its horizontal 3-tap line
    z = PP.nms_host(x, 20, 3.0)
    assert z.dtype == np.uint8 and set(np.unique(z).tolist()) <= {0, 255}
    assert (z[:, 15] == 255).all()
    # columns 14 and 16 are below their neighbour 15 horizontally and diagonally; vertically they form a constant line, which the
    # `==` rule keeps (dilate(x) == x on a plateau), and their blurred value 255 * g[1] is above the threshold too
    g = np.exp(-(np.arange(25) - 12.0) ** 2 / 18.0)
    g /= g.sum()
    assert 255 * g[11] > 20 and (z[:, 14] == 255).all()
    far = 255 * g[12 - 9]  # nine columns away the blurred value is below the threshold
    assert far < 20 and (z[:, 15 - 9] == 0).all()


def test_nms_plateau_and_threshold():
    x = np.full((9, 9), 100, dtype=np.uint8)  # a plateau: the blur of a constant is the constant, every pixel equals its dilation
    assert (PP.nms_host(x, 99, 3.0) == 255).all()
    assert (PP.nms_host(x, 100, 3.0) == 0).all()  # strictly greater than t
    with pytest.raises(ValueError):
        PP.nms_host(np.zeros((3, 3, 3), dtype=np.uint8), 1, 3.0)


def test_nms_slope_is_removed():
    x = np.tile(np.arange(0, 240, 6, dtype=np.uint8)[None, :], (40, 1))  # a horizontal ramp: maximal along the vertical line only
    z = PP.nms_host(x, 127, 3.0)
    blurred_ok = z[:, 30:38]  # values above 127 in the interior of the ramp survive through the vertical plateau rule
    assert (blurred_ok == 255).all() and (z[:, :15] == 0).all()


def test_fake_scribble_values_and_shape():
    e = np.zeros((40, 48), dtype=np.uint8)
    e[20, 8:40] = 255  # one bright line
    out = PP.fake_scribble_from_hed(e)
    assert out.shape == (40, 48, 3) and out.dtype == np.uint8
    assert set(np.unique(out).tolist()) <= {0, 255}
    assert np.array_equal(out[:, :, 0], out[:, :, 1]) and np.array_equal(out[:, :, 0], out[:, :, 2])
    assert (PP.fake_scribble_from_hed(np.zeros((20, 20), dtype=np.uint8)) == 0).all()
    with pytest.raises(ValueError):
        PP.fake_scribble_from_hed(np.zeros((20, 20, 3), dtype=np.uint8))


# ---- fixtures and the key contract -----------------------------------------------------------------------------------------------------------------
def test_fixtures_load_and_keys_match():
    from cremage_amd import annotator_hip
    m = annotator_hip.ControlNetHED_Apache2()
    sd = m.state_dict()
    sha, n = HC.key_digest(sd)
    assert n == HC.FULL_KEYS and sum(p.numel() for p in m.parameters()) == HC.FULL_PARAMS
    for name, (h, w) in HC.FULL_CASES.items():
        z, meta = _load("hed_" + name)
        assert meta["keys_sha1"] == sha and meta["n_keys"] == n and meta["n_params"] == HC.FULL_PARAMS
        for i in range(5):
            assert z[f"proj{i + 1}"].shape == (1, 1, h >> i, w >> i)
    for name, (args, shape, _) in HC.BLOCK_CASES.items():
        z, meta = _load("hed_" + name)
        b = annotator_hip.DoubleConvBlock(*args)
        assert meta["keys_sha1"] == HC.key_digest(b.state_dict())[0]
    assert set(sd) == {"norm"} | {f"block{k}.convs.{j}.{p}" for k, layers in enumerate(HC.LAYERS, 1) for j in range(layers) for p in ("weight", "bias")} | \
        {f"block{k}.projection.{p}" for k in range(1, 6) for p in ("weight", "bias")}
    renamed = {("block1.proj.weight" if k == "block1.projection.weight" else k): v for k, v in sd.items()}
    with pytest.raises(RuntimeError):
        m.load_state_dict(renamed, strict=True)
    m.load_state_dict(sd, strict=True)


def test_synthetic_fill_rule_is_the_pipelines():
    """pipeline.build_synthetic_hed and _hed_cases.fill_ must give the same weights (the fixtures are made with the latter)"""
    from cremage_amd import pipeline
    a = pipeline.build_synthetic_hed(device="cpu").state_dict()
    b = HC.build_full("cpu").state_dict()
    assert all(torch.equal(a[k], b[k]) for k in b) and set(a) == set(b)
