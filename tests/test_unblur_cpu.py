"""Face unblur / colorize without a GPU: the plain-torch restatement against the reference's own outputs, the parity formula of the
transposed conv against F.conv_transpose2d, the module tree against the reference's state-dict keys, and the host glue."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import _unblur_cases as UC
from tests.conftest import load_golden


# ------------------------------------------------------------------------------------------------------------- restatement vs fixtures
def _state_dict(cls, args, prefix):
    """the reference class's state dict, rebuilt from the drop-in of the same tree with the fixture's name-keyed weights"""
    from cremage_amd import unblur_hip
    from cremage_amd.synth import synth_fill_
    torch.manual_seed(0)
    m = getattr(unblur_hip, cls)(*args)
    synth_fill_(m, UC.SEED, prefix=prefix)
    return m, {k: v.detach() for k, v in m.state_dict().items()}


@pytest.mark.parametrize("name", list(UC.BLOCK_CASES))
def test_restatement_reproduces_block_fixture(name):
    meta, arrays = load_golden("unblur_" + name)
    cls, args, shape = UC.BLOCK_CASES[name]
    assert meta["cls"] == cls and meta["args"] == list(args) and meta["x"] == list(shape)
    m, sd = _state_dict(cls, args, meta["prefix"])
    assert UC.key_digest(sd) == (meta["keys_sha1"], meta["n_keys"])  # same tree and parameter names as the reference class
    assert sum(p.numel() for p in m.parameters()) == meta["n_params"]
    with torch.no_grad():
        y = UC.block_forward(name, UC.block_input(name), sd)
    own = meta["ref_fp32_vs_fp64"]["y"]
    rel = UC.rel_l2(y, arrays["y"])
    print(f"[fig] {name}: restatement vs fixture {rel:.3e}, the reference's own fp32 vs fp64 {own:.3e}")
    assert tuple(y.shape) == tuple(arrays["y"].shape)
    assert rel <= 4 * own, (name, rel, own)  # same primitives: only the summation order can differ


def test_full_model_tree_matches_the_reference_keys():
    """strict=True is a statement about keys and shapes: built on the meta device, the 620 M-parameter tree costs nothing"""
    from cremage_amd.unblur_hip import UnblurCremageModelV6
    meta, arrays = load_golden("unblur_full")
    with torch.device("meta"):
        m = UnblurCremageModelV6()
    sd = m.state_dict()
    assert UC.key_digest(sd) == (meta["keys_sha1"], meta["n_keys"])
    assert meta["n_keys"] == UC.FULL_KEYS and sum(p.numel() for p in m.parameters()) == meta["n_params"] == UC.FULL_PARAMS
    assert sorted(arrays) == sorted(["out", "mid"] + [f"h.{i}" for i in range(UC.TAPS)])
    for k, shape in meta["shapes"].items():
        assert arrays[k].numel() == min(UC.SAMPLE, math.prod(shape))


def test_restatement_reproduces_full_fixture():
    """the whole network, 620 M name-keyed weights drawn straight into a state dict (no module is built)"""
    from cremage_amd.synth import synth_tensor
    from cremage_amd.unblur_hip import UnblurCremageModelV6
    meta, arrays = load_golden("unblur_full")
    with torch.device("meta"):
        shapes = {k: tuple(v.shape) for k, v in UnblurCremageModelV6().state_dict().items()}
    sd = {k: synth_tensor(meta["prefix"] + k, s, UC.SEED) for k, s in shapes.items()}
    with torch.no_grad():
        out, taps, mid = UC.model_forward(UC.full_input(meta["batch"]), sd)
    got = {"out": out, "mid": mid, **{f"h.{i}": t for i, t in enumerate(taps)}}
    for k in sorted(arrays):
        assert list(got[k].shape) == meta["shapes"][k], k
        rel, own = UC.rel_l2(UC.sampled(got[k]), arrays[k]), meta["ref_fp32_vs_fp64"][k]
        print(f"[fig] full {k}: restatement vs fixture {rel:.3e}, the reference's own fp32 vs fp64 {own:.3e}")
        assert rel <= 4 * own, (k, rel, own)


def test_half_precision_raises_without_a_device():
    from cremage_amd.unblur_hip import ResnetSingleBlock, UnblurCremageModelV6
    with torch.device("meta"):
        m = UnblurCremageModelV6()
    with pytest.raises(NotImplementedError):
        m.half()
    with pytest.raises(NotImplementedError):
        m.bfloat16()
    blk = ResnetSingleBlock(16, 16).to(torch.bfloat16)
    with pytest.raises(NotImplementedError):
        blk(torch.zeros(1, 16, 4, 4))


# --------------------------------------------------------------------------------------------------------------------- parity formula
@pytest.mark.parametrize("hw", [(1, 1), (2, 3), (5, 7)], ids=["1x1", "2x3", "5x7"])
def test_parity_formula_is_conv_transpose(hw):
    n, cin, cout = 2, 6, 5
    x = torch.round(UC.synth(f"parity.x.{hw}", (n, cin) + hw, 3.0))
    w = torch.round(UC.synth(f"parity.w.{hw}", (cin, cout, 4, 4), 3.0))
    b = torch.round(UC.synth(f"parity.b.{hw}", (cout,), 3.0))
    assert float(x.abs().max()) * float(w.abs().max()) * 4 * cin < 2 ** 24  # integers: every sum is exact in fp32
    for bias in (None, b):
        assert torch.equal(UC.conv_transpose_parity(x, w, bias), F.conv_transpose2d(x, w, bias, stride=2, padding=1))
    # and the composed arm's weight: the same conv as ONE 3 x 3 conv with 4 Cout channels and a pixel shuffle
    w3, b3 = UC.composed_convt_weight(w, b)
    y = F.conv2d(x, w3, b3, padding=1)
    y = y.reshape(n, 2, 2, cout, hw[0], hw[1]).permute(0, 3, 4, 1, 5, 2).reshape(n, cout, 2 * hw[0], 2 * hw[1])
    assert torch.equal(y, F.conv_transpose2d(x, w, b, stride=2, padding=1))
    assert int((w3 != 0).sum()) <= 16 * cin * cout and w3.numel() == 36 * cin * cout  # 5 of 9 taps are structural zeros


# ------------------------------------------------------------------------------------------------------------------------- host glue
def _image(h, w, seed=0):
    return np.random.RandomState(seed).randint(1, 256, size=(h, w, 3)).astype(np.uint8)


def test_warp_identity_and_integer_shift():
    from cremage_amd import postprocess as PP
    img = _image(23, 31)
    ident = np.array([[1.0, 0.0, 0.0], [0.0, 1.0, 0.0]])
    assert np.array_equal(PP.warp_affine_u8(img, ident, 31, 23), img)
    # destination (x, y) reads source (x - 4, y + 3): pixels move right by 4 and up by 3, the uncovered border is zero
    out = PP.warp_affine_u8(img, np.array([[1.0, 0.0, -4.0], [0.0, 1.0, 3.0]]), 31, 23)
    want = np.zeros_like(img)
    want[:20, 4:] = img[3:, :27]
    assert np.array_equal(out, want)
    # a larger canvas: everything beyond the source is zero
    out = PP.warp_affine_u8(img, ident, 40, 30)
    assert np.array_equal(out[:23, :31], img) and not out[23:].any() and not out[:, 31:].any()


def test_warp_weights_are_integers_that_sum_to_one():
    from cremage_amd import postprocess as PP
    img = np.full((9, 9, 1), 200, dtype=np.uint8)
    m = np.array([[0.7, 0.2, 1.3], [-0.2, 0.7, 2.1]])
    out = PP.warp_affine_u8(img, m, 6, 6)
    inside = out[out > 0]
    assert inside.size and (inside[(inside == 200)].size > 0)  # a constant stays constant wherever all four taps are inside
    ax, bx, x0, y0 = PP.warp_affine_tables(m, 6, 6)
    assert all(t.dtype == np.int64 for t in (ax, bx, x0, y0)) and x0[0] == int(np.rint(1.3 * 1024)) + 16


def test_erosion_rule_at_the_border():
    from cremage_amd import postprocess as PP
    full = np.ones((7, 9, 1), dtype=bool)
    assert PP.erode5_mask(full).all()  # pixels outside the image do not constrain
    hole = full.copy()
    hole[0, 0] = False
    er = PP.erode5_mask(hole)
    assert not er[:3, :3].any() and er[3:].all() and er[:, 3:].all()
    lone = np.zeros((7, 9, 1), dtype=bool)
    lone[2:7, 4:9] = True  # a 5 x 5 block touching the bottom-right corner: rows / columns beyond the image count as set
    er = PP.erode5_mask(lone)
    want = np.zeros_like(lone)
    want[4:7, 6:9] = True
    assert np.array_equal(er, want)


def test_paste_leaves_everything_outside_the_eroded_mask_untouched():
    from cremage_amd import postprocess as PP
    img = _image(97, 131, 1)
    face = _image(256, 256, 2)
    face[100:110, 100:110] = 0  # zero bytes inside the face: holes of the mask
    th, s = math.radians(30.0), 0.7
    m = np.array([[s * math.cos(th), -s * math.sin(th), 40.0], [s * math.sin(th), s * math.cos(th), -20.0]])  # image -> face
    out = PP.paste_warped_face(img, face, m)
    warped = PP.warp_affine_u8(face, m, 131, 97)
    mask = PP.erode5_mask(warped > 0)
    assert mask.any() and not mask.all()
    assert np.array_equal(out[~mask], img[~mask]) and np.array_equal(out[mask], warped[mask])
    assert out is not img and out.dtype == np.uint8


def test_similarity_fit_recovers_a_known_transform():
    from cremage_amd import postprocess as PP
    tpl = np.array(PP.UNBLUR_LANDMARKS_256)
    assert tpl.shape == (5, 2) and abs(tpl[0, 0] - (38 + 30.2946) * 256 / 172) < 1e-12
    # integer landmarks (the fit truncates them), a template made from them by a known rotation, scale and shift
    pts = np.array([[120, 80], [180, 84], [150, 121], [127, 160], [171, 163]], dtype=np.float64)
    th, s, t = math.radians(-17.0), 1.37, np.array([-33.25, 12.5])
    a, b = s * math.cos(th), s * math.sin(th)
    want = np.array([[a, -b, t[0]], [b, a, t[1]]])
    q = pts @ want[:, :2].T + t
    got = PP.similarity_from_landmarks(pts + 0.75, template=q)  # + 0.75: truncated away, as astype(np.int32) does
    assert np.abs(got - want).max() < 1e-9
    inv = PP.invert_affine(got)
    assert np.abs(inv[:, :2] @ got[:, :2] - np.eye(2)).max() < 1e-12 and np.abs(inv[:, :2] @ got[:, 2] + inv[:, 2]).max() < 1e-9


def test_unblur_faces_host_with_a_stub_model():
    """identity model: the pasted pixels are the face's own, warped there and back; everything outside the pasted regions is untouched"""
    from cremage_amd import postprocess as PP
    img = _image(160, 200, 3)
    lms = [np.array(PP.UNBLUR_LANDMARKS_256) * 0.3 + [20, 10], np.array(PP.UNBLUR_LANDMARKS_256) * 0.25 + [110, 70]]
    calls = []

    def model(x):
        calls.append(tuple(x.shape))
        assert x.dtype == torch.float32 and 0.0 <= float(x.min()) and float(x.max()) <= 1.0
        return x * 1.5 - 0.1  # leaves [0, 1]: the glue clamps

    out = PP.unblur_faces(img, lms, model)
    assert calls == [(1, 3, 256, 256)] * 2 and out.shape == img.shape
    touched = np.zeros(img.shape, dtype=bool)
    for lm in lms:
        m = PP.similarity_from_landmarks(lm)
        touched |= PP.erode5_mask(PP.warp_affine_u8(np.full((256, 256, 3), 255, np.uint8), m, 200, 160) > 0)
    assert touched.any() and np.array_equal(out[~touched], img[~touched]) and (out != img).any()
    assert np.array_equal(PP.colorize_faces(img, lms, model), out)
