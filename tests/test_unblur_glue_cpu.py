"""The host side of the device glue of face unblur / colorize, without a GPU: `postprocess.warped_footprint` holds every non-zero pixel of
the warp it stands for, and `pipeline.unblur_faces` refuses what the device arm cannot do."""
import math

import numpy as np
import pytest
import torch

from cremage_amd import pipeline, postprocess as PP
from cremage_amd._lib import CrgError


def _sim(deg, s, tx, ty):
    c, k = s * math.cos(math.radians(deg)), s * math.sin(math.radians(deg))
    return np.array([[c, -k, tx], [k, c, ty]], dtype=np.float64)


def _sweep(count, seed, W, H, fw, fh):
    """seeded image -> face similarity maps: scale 0.05 .. 40 (log-uniform), any angle, and a shift that puts the face's centre anywhere
    from well inside the image to well outside it (partly or wholly outside)"""
    rs = np.random.RandomState(seed)
    for _ in range(count):
        s = math.exp(rs.uniform(math.log(0.05), math.log(40.0)))
        m = _sim(rs.uniform(0.0, 360.0), s, 0.0, 0.0)
        # the image point that lands on the face's centre: within 1.5 image sizes around the image's centre
        p = np.array([rs.uniform(-1.0, 2.0) * W, rs.uniform(-1.0, 2.0) * H])
        m[:, 2] = np.array([fw / 2.0, fh / 2.0]) - m[:, :2] @ p
        yield m


@pytest.mark.parametrize("W,H", [(40, 40), (83, 61)])
def test_footprint_holds_every_nonzero_pixel(W, H):
    fw, fh = 24, 20
    face = np.full((fh, fw, 1), 255, np.uint8)
    hit = empty = partial = 0
    for m in _sweep(200, 17 + W, W, H, fw, fh):
        warped = PP.warp_affine_u8(face, m, W, H)[:, :, 0] > 0
        x, y, w, h = PP.warped_footprint(m, (fw, fh), (W, H))
        assert 0 <= x and 0 <= y and x + w <= W and y + h <= H and w >= 0 and h >= 0, (m, (x, y, w, h))
        inside = np.zeros((H, W), dtype=bool)
        inside[y:y + h, x:x + w] = True
        assert not (warped & ~inside).any(), (m, (x, y, w, h), np.argwhere(warped & ~inside)[:4])
        hit += bool(warped.any())
        empty += (w == 0)
        partial += bool(warped.any() and not warped.all())
    # the sweep reaches all three situations: faces that cover pixels, faces cut by the border or smaller than the image, faces outside
    assert hit >= 50 and partial >= 30 and empty >= 10, (hit, partial, empty)


def test_footprint_is_not_the_whole_image_for_a_small_face():
    # a 256 x 256 face magnified 8 x lands on 32 x 32 image pixels around (100, 60) of a 300 x 200 image
    m = _sim(0.0, 8.0, -8.0 * 100, -8.0 * 60)
    x, y, w, h = PP.warped_footprint(m, (256, 256), (300, 200))
    assert (x, y) in [(99, 59), (98, 58)] and 33 <= w <= 36 and 33 <= h <= 36, (x, y, w, h)
    warped = PP.warp_affine_u8(np.full((256, 256, 1), 255, np.uint8), m, 300, 200)[:, :, 0] > 0
    ys, xs = np.nonzero(warped)
    assert x <= xs.min() and xs.max() < x + w and y <= ys.min() and ys.max() < y + h


@pytest.mark.parametrize("m", [
    [[0.0, 0.0, 3.0], [0.0, 0.0, 4.0]],                # singular: every pixel reads the same source point
    [[1e-200, 0.0, 3.0], [0.0, 1e-200, 4.0]],          # the determinant underflows to 0
    [[1.0, 2.0, 0.0], [0.5, 1.0, 0.0]],                # rank one
    [[1e15, 0.0, 0.0], [0.0, 1e15, 0.0]],              # table entries reach the 2^40 clip
    [[float("nan"), 0.0, 0.0], [0.0, 1.0, 0.0]],
    [[1.0, 0.0, float("inf")], [0.0, 1.0, 0.0]],
])
def test_footprint_of_a_map_it_cannot_reason_about_is_the_whole_image(m):
    assert PP.warped_footprint(m, (16, 16), (40, 30)) == (0, 0, 40, 30)


class _Stub(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.a = torch.nn.Parameter(torch.tensor(1.5))

    def forward(self, x):
        return x * self.a - 0.1


def test_device_glue_needs_a_device_model_and_a_known_glue():
    img = np.random.RandomState(0).randint(1, 256, size=(64, 80, 3)).astype(np.uint8)
    lms = [np.array(PP.UNBLUR_LANDMARKS_256) * 0.2 + [10, 5]]
    model = _Stub()
    with pytest.raises(CrgError):
        pipeline.unblur_faces(model, img, lms, glue="device")
    with pytest.raises(CrgError):
        pipeline.colorize_faces(model, img, lms, glue="device")
    with pytest.raises(CrgError):
        pipeline.unblur_faces(model, img, lms, graph=True)
    with pytest.raises(ValueError):
        pipeline.unblur_faces(model, img, lms, glue="gpu")
    # the host arm is what it was
    out = pipeline.unblur_faces(model, img, lms)
    assert isinstance(out, np.ndarray) and np.array_equal(out, PP.unblur_faces(img, lms, model))
    assert np.array_equal(pipeline.colorize_faces(model, img, lms), out)
