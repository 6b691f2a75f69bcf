"""The device glue of face unblur / colorize against its host definitions, byte for byte: ops.warp_affine_u8 against
postprocess.warp_affine_u8, ops.paste_warped_u8 against postprocess.paste_warped_face, pipeline.unblur_faces(glue="device") against the host
arm, and the graph replay of the model call against the eager call.  Everything here is integer arithmetic or one correctly rounded fp32
operation, so every comparison is equality."""
import math

import numpy as np
import pytest
import torch

from cremage_amd import ops, pipeline, postprocess as PP
from cremage_amd._lib import CrgError

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
IDENT = [[1.0, 0.0, 0.0], [0.0, 1.0, 0.0]]


def _bytes(seed, *shape):
    return np.random.RandomState(seed).randint(1, 256, size=shape).astype(np.uint8)


def _sim(deg, s, tx, ty):
    c, k = s * math.cos(math.radians(deg)), s * math.sin(math.radians(deg))
    return np.array([[c, -k, tx], [k, c, ty]], dtype=np.float64)


def _unit(host_u8):
    """what the host arm feeds the network: bytes / 255 in fp32, [C, H, W]"""
    return torch.from_numpy(host_u8).float().div(255).permute(2, 0, 1)


def _check_warp(src_np, maps, W, H, src_dev=None):
    """both output forms of one call against the host definition, map by map"""
    src_dev = torch.from_numpy(src_np).to(DEV) if src_dev is None else src_dev
    maps = np.asarray(maps, dtype=np.float64)
    batched = maps.ndim == 3
    want = [PP.warp_affine_u8(src_np, m, W, H) for m in (maps if batched else maps[None])]
    got = ops.warp_affine_u8(src_dev, maps, (W, H))
    assert got.dtype == torch.uint8 and tuple(got.shape) == ((len(want), H, W, src_np.shape[2]) if batched else (H, W, src_np.shape[2]))
    got = got.cpu().numpy()
    gotf = ops.warp_affine_u8(src_dev, torch.from_numpy(maps), (W, H), out_dtype=torch.float32)
    assert gotf.dtype == torch.float32 and tuple(gotf.shape) == (len(want), src_np.shape[2], H, W)
    gotf = gotf.cpu()
    for i, w in enumerate(want):
        assert np.array_equal(got[i] if batched else got, w), i
        assert torch.equal(gotf[i], _unit(w)), i
    return want


# ------------------------------------------------------------------------------------------------------------------------------ warp
@pytest.mark.parametrize("m,W,H", [(IDENT, 31, 23), ([[1.0, 0.0, -4.0], [0.0, 1.0, 3.0]], 31, 23), (IDENT, 40, 30)], ids=["identity", "shift", "canvas"])
def test_warp_identity_shift_canvas(m, W, H):
    src = _bytes(1, 23, 31, 3)
    want = _check_warp(src, m, W, H)[0]
    if (W, H) == (40, 30):
        assert np.array_equal(want[:23, :31], src) and not want[23:].any() and not want[:, 31:].any()
    elif m == IDENT:
        assert np.array_equal(want, src)


def test_warp_one_channel_affine():
    _check_warp(_bytes(2, 9, 9, 1), [[0.7, 0.2, 1.3], [-0.2, 0.7, 2.1]], 6, 6)


def test_warp_magnifying_align():
    want = _check_warp(_bytes(3, 61, 83, 3), PP.invert_affine(_sim(30.0, 5.0, -60.0, -160.0)), 256, 256)[0]
    assert (want > 0).any()


def test_warp_64_maps_in_one_call_rgba_and_its_rgb_view():
    rs = np.random.RandomState(4)
    maps = np.concatenate([rs.uniform(-3.0, 3.0, size=(64, 2, 2)), rs.uniform(-20.0, 20.0, size=(64, 2, 1))], axis=2)
    src = _bytes(5, 13, 11, 4)
    dev = torch.from_numpy(src).to(DEV)
    want = _check_warp(src, maps, 19, 17, dev)
    assert sum(bool(w.any()) for w in want) >= 32
    _check_warp(np.ascontiguousarray(src[:, :, :3]), maps, 19, 17, dev[:, :, :3])
    assert torch.equal(dev.cpu(), torch.from_numpy(src))


@pytest.mark.parametrize("m", [[[1e15, 0.0, 0.0], [0.0, 1e15, 0.0]], [[2.0 ** 29, 0.0, -3.0], [0.0, 1.0, 0.0]]], ids=["1e15", "2^29"])
def test_warp_positions_beyond_int32(m):
    want = _check_warp(_bytes(6, 12, 10, 3), m, 8, 8)[0]
    rest = want.copy()
    rest[0, 0] = 0
    assert not rest.any()  # only (0, 0) may read the source: every other pixel lies 2^29 pixels or more outside it
    if m[0][2] == 0.0:
        assert np.array_equal(want[0, 0], _bytes(6, 12, 10, 3)[0, 0])  # (0, 0) sits on source pixel (0, 0)


def test_warp_windows_and_guard_bands():
    big = _bytes(7, 40, 50, 3)
    bigd = torch.from_numpy(big).to(DEV)
    m = [[0.9, -0.3, 2.0], [0.3, 0.9, -1.5]]
    want = PP.warp_affine_u8(np.ascontiguousarray(big[5:28, 7:38]), m, 20, 14)
    canvas = torch.full((30, 36, 3), 77, dtype=torch.uint8, device=DEV)
    ret = ops.warp_affine_u8(bigd[5:28, 7:38], m, (20, 14), out=canvas[9:23, 11:31])
    assert ret.data_ptr() == canvas[9:23, 11:31].data_ptr()
    got = canvas.cpu().numpy()
    assert np.array_equal(got[9:23, 11:31], want)
    got[9:23, 11:31] = 77
    assert (got == 77).all()
    assert torch.equal(bigd.cpu(), torch.from_numpy(big))
    # fp32 into a window of a larger planar buffer
    plane = torch.full((2, 3, 20, 26), -5.0, device=DEV)
    ops.warp_affine_u8(bigd[5:28, 7:38], [m, IDENT], (20, 14), out=plane[:, :, 3:17, 2:22])
    p = plane.cpu()
    assert torch.equal(p[0, :, 3:17, 2:22], _unit(want))
    p[:, :, 3:17, 2:22] = -5.0
    assert (p == -5.0).all()


# ------------------------------------------------------------------------------------------------------------------------------ paste
def _face(seed, ch=3):
    face = _bytes(seed, 256, 256, ch)
    face[100:140, 90:130] = 0  # holes of the mask
    return face


def _check_paste(image_np, face_np, m, face_dev=None, image_dev=None):
    """rect=None and rect = the whole image against the host paste; returns the host result"""
    want = PP.paste_warped_face(image_np, face_np, m)
    H, W = image_np.shape[:2]
    face_dev = torch.from_numpy(face_np).to(DEV) if face_dev is None else face_dev
    for rect in (None, (0, 0, W, H)):
        img = torch.from_numpy(image_np).to(DEV) if image_dev is None else image_dev(image_np)
        v = img._version
        ret = ops.paste_warped_u8(img, face_dev, m, rect=rect)
        assert ret is img and img._version > v
        assert np.array_equal(img.cpu().numpy(), want), rect
    return want


PASTE_CASES = {
    "inside": ((61, 83), (30.0, 5.0, -60.0, -160.0)),
    "corner": ((61, 83), (-20.0, 4.0, 40.0, -30.0)),
    "magnified": ((300, 420), (10.0, 0.6, -20.0, -10.0)),
    "vanishes": ((40, 40), (0.0, 64.0, -1000.0, -1000.0)),
}


@pytest.mark.parametrize("name", list(PASTE_CASES))
def test_paste_cases(name):
    (H, W), sim = PASTE_CASES[name]
    image, face, m = _bytes(11, H, W, 3), _face(12), _sim(*sim)
    want = _check_paste(image, face, m)
    changed = PP.erode5_mask(PP.warp_affine_u8(face, m, W, H) > 0)
    print(f"[fig] {name}: the eroded mask covers {changed.mean():.2%} of the bytes, footprint {PP.warped_footprint(m, (256, 256), (W, H))}")
    if name == "vanishes":
        assert not changed.any() and np.array_equal(want, image)
    else:
        assert changed.any() and not changed.all()


@pytest.mark.parametrize("ch", [1, 4])
def test_paste_channel_counts(ch):
    _check_paste(_bytes(13, 61, 83, ch), _face(14, ch), _sim(30.0, 5.0, -60.0, -160.0))


def test_paste_into_a_window_leaves_the_guard_band():
    image, face, m = _bytes(15, 61, 83, 3), _face(16), _sim(-20.0, 4.0, 40.0, -30.0)
    holders = []

    def window(image_np):
        big = torch.full((75, 100, 4), 99, dtype=torch.uint8, device=DEV)
        big[6:67, 9:92, :3] = torch.from_numpy(image_np).to(DEV)
        holders.append(big)
        return big[6:67, 9:92, :3]
    _check_paste(image, face, m, image_dev=window)
    for big in holders:
        g = big.cpu().numpy()
        g[6:67, 9:92, :3] = 99
        assert (g == 99).all()


def test_paste_fp32_face_is_quantised_like_the_host():
    y = torch.from_numpy(np.random.RandomState(17).uniform(-0.2, 1.3, size=(1, 3, 256, 256)).astype(np.float32))
    y[0, :, 100:140, 90:130] = -0.05  # quantises to 0: holes
    face = PP._unit_to_face(y)
    assert face.min() == 0 and face.max() == 255
    image, m = _bytes(18, 61, 83, 3), _sim(30.0, 5.0, -60.0, -160.0)
    yd = y.to(DEV)
    _check_paste(image, face, m, face_dev=yd[0])
    _check_paste(image, face, m, face_dev=yd)
    _check_paste(image, face, m, face_dev=yd.contiguous(memory_format=torch.channels_last))


# ------------------------------------------------------------------------------------------------------------------------------ chain
class _Stub(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.a = torch.nn.Parameter(torch.tensor(1.5))

    def forward(self, x):
        return x * self.a - 0.1


def test_chain_with_a_stub_model_equals_the_host_arm():
    model = _Stub().to(DEV)
    img = _bytes(19, 160, 200, 3)
    tpl = np.array(PP.UNBLUR_LANDMARKS_256)
    lms = [tpl * 0.3 + [20, 10], tpl * 0.25 + [60, 30]]
    want = pipeline.unblur_faces(model, img, lms, glue="host")
    assert isinstance(want, np.ndarray) and (want != img).any()
    got = pipeline.unblur_faces(model, img, lms, glue="device")
    assert torch.is_tensor(got) and got.is_cuda and got.dtype == torch.uint8 and tuple(got.shape) == img.shape
    assert np.array_equal(got.cpu().numpy(), want)
    dev = torch.from_numpy(img).to(DEV)
    got2 = pipeline.unblur_faces(model, dev, lms, glue="device")
    assert got2.data_ptr() != dev.data_ptr() and np.array_equal(got2.cpu().numpy(), want)
    assert np.array_equal(dev.cpu().numpy(), img)  # the caller's tensor is unchanged
    assert np.array_equal(pipeline.colorize_faces(model, dev, lms, glue="device").cpu().numpy(), want)
    # the second face's paste overlaps the first one's: the order of the host loop is part of the result
    one = pipeline.unblur_faces(model, img, lms[1:], glue="host")
    assert (one != want).any()


# ------------------------------------------------------------------------------------------------------------------------- full model
@pytest.fixture(scope="module")
def full_model():
    from tests import _unblur_cases as UC
    return pipeline.build_synthetic_unblur(DEV, UC.SEED)


@pytest.fixture(scope="module")
def full_case(full_model):
    img = _bytes(5, 300, 420, 3)
    tpl = np.array(PP.UNBLUR_LANDMARKS_256)
    lms = [tpl * 0.5 + [30, 20], tpl * 0.4 + [250, 150]]
    return img, lms, pipeline.unblur_faces(full_model, img, lms, glue="host")


def test_full_model_device_arm_equals_host_arm(full_model, full_case):
    img, lms, want = full_case
    got = pipeline.unblur_faces(full_model, img, lms, glue="device")
    assert got.is_cuda and np.array_equal(got.cpu().numpy(), want)
    assert (want != img).any()


def test_full_model_graph_replay_equals_eager(full_model, full_case):
    img, lms, want = full_case
    got = pipeline.unblur_faces(full_model, img, lms, glue="device", graph=True)
    g = full_model._crg_graphed
    assert np.array_equal(got.cpu().numpy(), want)
    assert g.captures == 1 and g.replays >= 1 and not g.broken
    # other landmarks, and the host arm: the same capture is replayed
    tpl = np.array(PP.UNBLUR_LANDMARKS_256)
    lms2 = [tpl * 0.45 + [120, 60]]
    replays = g.replays
    got2 = pipeline.unblur_faces(full_model, img, lms2, glue="host", graph=True)
    assert full_model._crg_graphed is g and g.captures == 1 and g.replays == replays + 1
    assert np.array_equal(got2, pipeline.unblur_faces(full_model, img, lms2, glue="host"))
    # the replay's output against the eager call's, on the network's own output
    x = ops.warp_affine_u8(torch.from_numpy(img).to(DEV), PP.invert_affine(PP.similarity_from_landmarks(lms2[0])), (256, 256), out_dtype=torch.float32)
    assert torch.equal(g(x), full_model(x)) and g.captures == 1


# ------------------------------------------------------------------------------------------------------------------------------ errors
def test_errors_are_raised_before_any_launch():
    src = torch.from_numpy(_bytes(20, 12, 10, 3)).to(DEV)
    face = torch.from_numpy(_bytes(21, 16, 16, 3)).to(DEV)
    image = torch.from_numpy(_bytes(22, 20, 24, 3)).to(DEV)
    before = image.clone()
    with pytest.raises(CrgError):
        ops.warp_affine_u8(src.cpu(), IDENT, (8, 8))
    with pytest.raises(CrgError):
        ops.paste_warped_u8(image.cpu(), face.cpu(), IDENT)
    with pytest.raises(CrgError):
        ops.paste_warped_u8(image, face.cpu(), IDENT)
    five = torch.zeros((12, 10, 5), dtype=torch.uint8, device=DEV)
    with pytest.raises(CrgError):
        ops.warp_affine_u8(five, IDENT, (8, 8))
    with pytest.raises(CrgError):
        ops.paste_warped_u8(five, five, IDENT)
    planar = torch.zeros((3, 12, 10), dtype=torch.uint8, device=DEV).permute(1, 2, 0)  # [h, w, C] whose channels are a plane apart
    with pytest.raises(CrgError):
        ops.warp_affine_u8(planar, IDENT, (8, 8))
    with pytest.raises(CrgError):
        ops.paste_warped_u8(planar[:, :, :3], face, IDENT)
    with pytest.raises(CrgError):
        ops.warp_affine_u8(src, IDENT, (8, 8), out=torch.zeros((3, 8, 8), dtype=torch.uint8, device=DEV).permute(1, 2, 0))
    for bad in (float("nan"), float("inf")):
        m = [[1.0, 0.0, bad], [0.0, 1.0, 0.0]]
        with pytest.raises(CrgError):
            ops.warp_affine_u8(src, [IDENT, m], (8, 8))
        with pytest.raises(CrgError):
            ops.paste_warped_u8(image, face, m)
        with pytest.raises(CrgError):
            ops.paste_warped_u8(image, face, m, rect=(0, 0, 24, 20))
    with pytest.raises(CrgError):
        ops.warp_affine_u8(src, IDENT, (0, 8))
    with pytest.raises(CrgError):
        ops.paste_warped_u8(image, face, IDENT, rect=(10, 10, 20, 20))  # a rectangle that leaves the image
    with pytest.raises(CrgError):
        ops.paste_warped_u8(image, torch.zeros((4, 16, 16), device=DEV), IDENT)  # 4 planes for 3 channels
    assert torch.equal(image, before)
